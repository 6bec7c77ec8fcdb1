"""Cache adaptation (TKZ_OPT_ADAPT) on the PIPELINED host path: tkz_encode_batch_utf8 / _utf16 calls that HostPipeline (tkz_api.cpp) cuts into
chunks on two leased workspaces, two launch sequences in flight -- every chunk a batch of its own to the policy (tkz_adapt.h).  parity.check_adaptation and
check_memo_refresh pin the rule where a call is ONE batch; these scenarios cross it with the pipeline.  Shared by tests/test_emu_adapt_host.py (the CPU-emulated
build) and tests/test_gpu_adapt_host.py.

The chunk size ($TKZ_HOST_CHUNK_BYTES) and the policy's distances ($TKZ_ADAPT_*) are read once per process / per encoder: every scenario runs in a child
interpreter -- this file as a script, `adapt_host_cases.py SCENARIO emu|gpu` -- which child() starts with the environment of child_env().  The text is
check_adaptation's (parity.adapt_lexicons / adapt_batch): the gpt2 table, the cl100k pattern, TKZ_OPT_PROMOTE_MIN_BYTES 100,000, batches of 160 KB + up to one
document, so 2 or 3 chunks of 64 KiB a call.  Every batch of every scenario is compared with the oracle, ids and offsets, exactly.

THE CUT IS MADE VISIBLE by $TKZ_TRACE_HOST: the pipeline prints one line, "[tkz host trace] N chunks: ...", for every call of more than one chunk (and none
for a call that went as one).  The child points its stderr at a file (Tap) and reads the lines of every call back: a scenario asserts, call by call, that the
call was cut -- were it not, the run would only prove the one-chunk path again.  (On the device with page-locked buffers Encoder.engine_downloads tells the same
where the copy engine is available; it is printed, not asserted: the path is optional by design, tkz_sdma.h.)

The child prints one JSON line per batch -- adapt_stats() read after it, which waits for an install or a drop in flight on its thread -- and `ADAPT_HOST_OK` last.
The bounds are check_adaptation's own: a re-learn counted within 4 batches of a change of text (its `seen_relearn <= 3`), more than 50 promoted pieces (the
one-chunk path gives 284 on this text), the workspace within 4 MB.  Promotions are back within 3 batches of the re-learn: the one-chunk path needs 1, the pipeline
gets 2 more, because a window that needs the memo emptied can only open where the call's sibling workspace has nothing in flight -- chunk 0 --, so it may wait
for the next call's first chunk, and a window of 100,000 bytes is two chunks of the workspace that holds the slot, every other chunk of the call."""
import ctypes as C
import gzip
import json
import os
import random
import re
import subprocess
import sys
import tempfile
import threading

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CHUNK_BYTES = 65536
MIN_PROMOTED = 50            # check_adaptation's bound
RELEARN_WITHIN = 4           # batches from a change of text to the re-learn being counted (check_adaptation: seen_relearn <= 3)
PROMOTED_WITHIN = 3          # batches from the re-learn to promotions again
SCENARIOS = ["stationary", "drift_and_back", "page_locked", "utf16", "two_callers", "full_list_one_chunk", "full_list_pipelined", "memo_three_quarters"]


def child_env(scenario):
    """the environment of a scenario's child: the caller's without any TKZ_ADAPT_* / chunk / memo setting, plus the scenario's own"""
    env = {k: v for k, v in os.environ.items() if not (k.startswith("TKZ_ADAPT_") or k in ("TKZ_HOST_CHUNK_BYTES", "TKZ_MEMO_SLOTS_LOG2", "TKZ_TRACE_HOST"))}
    env.update(TKZ_ADAPT_SETTLE_BYTES="100000", TKZ_ADAPT_MIN_BYTES="300000", TKZ_TRACE_HOST="1")
    if scenario != "full_list_one_chunk":
        env["TKZ_HOST_CHUNK_BYTES"] = str(CHUNK_BYTES)
    if scenario == "memo_three_quarters":          # check_memo_refresh's settings (it sets them itself where it runs in the suite's own process)
        env.update(TKZ_MEMO_SLOTS_LOG2="12", TKZ_ADAPT_ROUND_BYTES="300000")
    return env


def child(scenario, backend, timeout):
    """runs one scenario in a child interpreter; returns its output (the per-batch series) or fails with the end of what it wrote"""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), scenario, backend], env=child_env(scenario), capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and "ADAPT_HOST_OK " + scenario in out.stdout, "%s: exit %s\n%s\n%s" % (scenario, out.returncode, out.stdout[-6000:], out.stderr[-3000:])
    print(out.stdout)
    return out.stdout


# ---- in the child --------------------------------------------------------------------------------------------------------------------------

class Tap:
    """the process's stderr in a file: the lines $TKZ_TRACE_HOST wrote since the last look.  close() puts stderr back and passes everything on."""
    LINE = re.compile(r"\[tkz host trace\] (\d+) chunks:")

    def __init__(self):
        self.file = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.file.fileno(), 2)
        self.pos = 0

    def chunks(self):
        """the chunk counts of the pipelined calls since the last look, one entry a call"""
        sys.stderr.flush()
        self.file.seek(self.pos)
        new = self.file.read()
        self.pos += len(new)
        return [int(m.group(1)) for m in self.LINE.finditer(new.decode("utf-8", "replace"))]

    def close(self):
        sys.stderr.flush()
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.file.seek(0)
        rest = self.file.read().decode("utf-8", "replace")
        sys.stderr.write("\n".join(ln for ln in rest.splitlines() if not self.LINE.search(ln))[-8000:] + "\n")
        self.file.close()


class HostBuffers:
    """page-locked buffers (tkz_host_alloc) for the text, its offsets, the ids and the result offsets of one batch"""
    def __init__(self, lib, max_bytes, max_docs):
        self.lib, self.max_bytes, self.max_docs = lib, max_bytes, max_docs
        self.p = [C.c_void_p() for _ in range(4)]
        for h, n in zip(self.p, [max_bytes + 64, 8 * (max_docs + 1), 4 * max_bytes + 64, 8 * (max_docs + 1)]):
            lib.check(lib.L.tkz_host_alloc(n, C.byref(h)))

    def encode(self, enc, data, offs):
        n = len(offs) - 1
        assert len(data) <= self.max_bytes and n <= self.max_docs
        offs64 = np.ascontiguousarray(offs, np.int64)
        C.memmove(self.p[0], data.ctypes.data, len(data))
        C.memmove(self.p[1], offs64.ctypes.data, 8 * (n + 1))
        needed = C.c_int64(0)
        self.lib.check(self.lib.L.tkz_encode_batch_utf8(enc._h, self.p[0], self.p[1], n, self.p[2], len(data), self.p[3], C.byref(needed)))
        return (np.ctypeslib.as_array(C.cast(self.p[2], C.POINTER(C.c_int32)), (max(needed.value, 1),))[:needed.value].copy(),
                np.ctypeslib.as_array(C.cast(self.p[3], C.POINTER(C.c_int64)), (n + 1,)).copy())

    def free(self):
        for h in self.p:
            self.lib.L.tkz_host_free(h)


class Run:
    """one encoder, its oracle, the tap; call() is one batch: encoded, compared, shown to have been cut, its adapt_stats() added to the series"""
    def __init__(self, lib, N, O, raw, tap, how="pageable", pipelined=True, cap=None):
        import parity
        self.parity, self.N, self.O, self.lib, self.tap, self.how, self.pipelined = parity, N, O, lib, tap, how, pipelined
        self.ovocab = O.Vocab(raw)
        self.oenc = O.Encoder(self.ovocab, N.CL100K)
        self.enc = N.Encoder(N.Vocab(raw, lib), N.CL100K)
        self.enc.set_option(N.OPT_PROMOTE_MIN_BYTES, 100_000)
        if cap is not None:
            self.enc.set_option(N.OPT_PROMOTE_CAP, cap)
        self.lex = dict(zip("AB", parity.adapt_lexicons()))
        self.rng = random.Random(71 + 3)
        self.bufs = HostBuffers(lib, 200_000, 1024) if how == "page_locked" else None
        self.series = []

    def encode(self, docs, enc=None, oenc=None):
        """-> nothing; raises where ids or offsets are not the oracle's"""
        enc, oenc = enc or self.enc, oenc or self.oenc
        data, offs = self.parity.pack(docs)
        if self.how == "utf16":                            # (the text is ASCII: a code unit a byte)
            ids, ooff = enc.encode_batch_utf16(data.astype(np.uint16), offs)
            e, eo = [], [0]
            for d in docs:
                e += oenc.encode_utf16(np.frombuffer(d, np.uint8).astype(np.uint16))
                eo.append(len(e))
        else:
            ids, ooff = self.bufs.encode(enc, data, offs) if self.bufs else enc.encode_batch(data, offs)
            e, eo = self.parity.oracle_encode_docs(oenc, docs)
        assert ids.tolist() == e and ooff.tolist() == eo, "ids or offsets differ from the oracle's"

    def call(self, text):
        docs = self.parity.adapt_batch(self.lex[text], self.rng)
        self.encode(docs)
        cut = self.tap.chunks()
        if self.pipelined:
            assert len(cut) == 1 and cut[0] >= 2, "the call was not cut into chunks: %r (%d bytes)" % (cut, sum(map(len, docs)))
        else:
            assert cut == [], "a call meant for the one-chunk path was cut: %r" % (cut,)
        st = self.enc.adapt_stats()
        st.update(i=len(self.series), text=text, chunks=cut[0] if cut else 1, workspace_bytes=self.enc.workspace_bytes)
        self.series.append(st)
        print(json.dumps({k: st[k] for k in ("i", "text", "chunks", "promotions", "relearns", "promoted_pieces", "settled_miss_share", "recent_miss_share", "retired_images")}), flush=True)
        return st

    def leg(self, text, n):
        return [self.call(text) for _ in range(n)]

    def drift_leg(self, text, n, relearns_before):
        """n batches of another text than the encoder has learnt: the re-learn is counted within RELEARN_WITHIN batches, more than MIN_PROMOTED pieces are
        promoted again within PROMOTED_WITHIN batches of it"""
        sts = self.leg(text, n)
        seen = next((k for k, st in enumerate(sts) if st["relearns"] > relearns_before), None)
        assert seen is not None and seen < RELEARN_WITHIN, "no re-learn within %d batches of the change to %s: %r" % (RELEARN_WITHIN, text, [st["relearns"] for st in sts])
        back = next((k for k, st in enumerate(sts) if k > seen and st["promoted_pieces"] > MIN_PROMOTED), None)
        assert back is not None and back - seen <= PROMOTED_WITHIN, \
            "no promotions within %d batches of the re-learn (batch %d of the leg): %r" % (PROMOTED_WITHIN, seen, [st["promoted_pieces"] for st in sts])
        return sts

    def finish(self):
        if self.bufs:
            self.bufs.free()


def stationary(mk):
    """14 batches of text A, pageable buffers: the encoder learns it and keeps what it learnt -- no re-learn on unchanged text"""
    r = mk()
    sts = r.leg("A", 14)
    # (the install lands on a thread: the first call may return before it -- and through the pipeline the first window may end in the second call)
    assert sts[2]["promotions"] >= 1, sts[2]
    assert sts[-1]["relearns"] == 0 and sts[-1]["promoted_pieces"] > MIN_PROMOTED, sts[-1]
    r.finish()


def drift_legs(r, back):
    sts = r.leg("A", 4)
    assert sts[-1]["relearns"] == 0 and sts[-1]["promoted_pieces"] > MIN_PROMOTED, sts[-1]
    mem0 = r.enc.workspace_bytes
    sts = r.drift_leg("B", 10, 0)
    if back:
        n = sts[-1]["relearns"]
        sts = r.drift_leg("A", 8, n)
        assert sts[-1]["relearns"] >= 2 and sts[-1]["promoted_pieces"] > MIN_PROMOTED, sts[-1]
        st = r.call("A")
        assert st["retired_images"] == 0, st                # freed when the call that followed the swap returned
        assert st["workspace_bytes"] <= mem0 + (4 << 20), (mem0, st["workspace_bytes"])
    r.finish()


def drift_and_back(mk):
    """4 x A, 10 x B, 8 x A: a re-learn at each change, promotions again after each, the replaced table images freed, the workspace no larger"""
    drift_legs(mk(), True)


def page_locked(mk):
    """A then B on tkz_host_alloc buffers for text, offsets, ids and result offsets: the path whose downloads leave by copy engine on hardware"""
    r = mk(how="page_locked")
    drift_legs(r, False)
    print(json.dumps({"engine_downloads": r.enc.engine_downloads}), flush=True)


def utf16(mk):
    """A then B through tkz_encode_batch_utf16 (the C# entry), against the oracle's UTF-16 entry"""
    drift_legs(mk(how="utf16"), False)


def two_callers(mk):
    """Two threads on one encoder, each sending pipelined batches (A, then B): another call really is in flight, so the memo must not be emptied under it --
    only exactness is asserted while both run.  Then one goes on with B alone: the re-learn and the promotions after it."""
    r = mk()
    errors = []

    def work(seed):
        try:
            oenc = r.O.Encoder(r.ovocab, r.N.CL100K)       # (the oracle's encoder keeps a cache of its own: one a thread)
            rng = random.Random(seed)
            for text in "AAAABBBB":
                r.encode(r.parity.adapt_batch(r.lex[text], rng), oenc=oenc)
        except BaseException as ex:                         # noqa: B036 -- reported by the main thread
            errors.append(repr(ex))
    threads = [threading.Thread(target=work, args=(s,)) for s in (101, 202)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    cut = r.tap.chunks()
    assert len(cut) == 16 and min(cut) >= 2, cut
    st = r.enc.adapt_stats()
    print(json.dumps({"after_both": {k: st[k] for k in ("promotions", "relearns", "promoted_pieces")}}), flush=True)
    sts = r.leg("B", RELEARN_WITHIN + PROMOTED_WITHIN)
    seen = next((k for k, s in enumerate(sts) if s["relearns"] >= 1), None)
    assert seen is not None and seen < RELEARN_WITHIN, [s["relearns"] for s in sts]
    # (a re-learn that fell into the time both ran counts from the first batch alone)
    start = seen if sts[seen]["relearns"] > st["relearns"] else -1
    back = next((k for k, s in enumerate(sts) if k > start and s["promoted_pieces"] > MIN_PROMOTED), None)
    assert back is not None and back - start <= PROMOTED_WITHIN, [s["promoted_pieces"] for s in sts]
    r.finish()


def full_list(mk, pipelined):
    """TKZ_OPT_PROMOTE_CAP 100: ONE window fills the list to its cap.  14 stationary batches keep it (it was dropped and learnt again every
    TKZ_ADAPT_MIN_BYTES, for ever); a full list still notices a real drift."""
    r = mk(cap=100, pipelined=pipelined)
    sts = r.leg("A", 14)
    assert sts[-1]["relearns"] == 0 and sts[-1]["promoted_pieces"] == 100, sts[-1]
    sts = r.leg("B", RELEARN_WITHIN)
    assert sts[-1]["relearns"] >= 1, [s["relearns"] for s in sts]
    r.finish()


def memo_three_quarters(lib, N, O, raw, tap):
    """parity.check_memo_refresh's scenario (a memo of 4,096 slots that text A fills; a learning round that reads it back three quarters full has it emptied before
    the next window -- the second way the policy comes to want the memo emptied) with every call cut into chunks.  Its assertion: merged[1] * 2 < merged[0].
    (Its count of the rounds text A sees is not asked here: without TKZ_OPT_ADAPT only a BATCH of the window's size learns, and a chunk of 64 KiB is none.)"""
    import parity
    vocab, oenc = N.Vocab(raw, lib), O.Encoder(O.Vocab(raw), N.CL100K)
    merged = {}
    for adapt in (1, 0):
        merged[adapt] = parity.memo_refresh_arm(lib, O, vocab, oenc, adapt, promotions_asserted=False)
        cut = tap.chunks()
        assert len(cut) == 6 + 10 + 1 and min(cut) >= 2, cut
    print(json.dumps({"merged_short": {"with the rule": merged[1], "without": merged[0]}}), flush=True)
    assert merged[1] * 2 < merged[0], merged


def main(scenario, backend):
    sys.path[:0] = [ROOT, TESTS]
    if backend == "gpu":
        import conftest  # noqa: F401 -- torch's HIP runtime initialises before libtkz is loaded
    from tokenizer_amd import _native as N
    from oracle import oracle as O
    O.build()
    if backend == "emu":
        import emu
        lib = emu.library()
    else:
        lib = N.default_library()
    with open(os.path.join(TESTS, "golden", "gpt2.tiktoken.gz"), "rb") as f:
        raw = gzip.decompress(f.read())
    tap = Tap()
    try:
        def mk(**kw):
            kw.setdefault("pipelined", scenario != "full_list_one_chunk")
            return Run(lib, N, O, raw, tap, **kw)
        if scenario == "memo_three_quarters":
            memo_three_quarters(lib, N, O, raw, tap)
        elif scenario.startswith("full_list_"):
            full_list(mk, scenario == "full_list_pipelined")
        else:
            {"stationary": stationary, "drift_and_back": drift_and_back, "page_locked": page_locked, "utf16": utf16, "two_callers": two_callers}[scenario](mk)
    finally:
        tap.close()
    print("ADAPT_HOST_OK " + scenario, flush=True)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
