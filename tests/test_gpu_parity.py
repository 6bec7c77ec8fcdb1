"""`-m gpu`: the parity tests proper.  Everything goes through the C ABI of the hipcc-built
tokenizer_amd/lib/libtkz.so on a real MI355X and is compared bit-exact with the CPU oracle, with the
reference's golden ids, and -- at sizes the oracle cannot reach in seconds -- through size-independent
properties (decode length = document length for every document, shard invariance, the two
pre-tokenizer formulations agreeing on the whole bitmap)."""
import os

import numpy as np
import pytest

import parity
from conftest import load_golden_json
from tokenizer_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return N.default_library()       # raises if libtkz.so is missing: no fallback


@pytest.fixture(scope="module")
def vocab(lib, gpt2_tiktoken_bytes):
    return N.Vocab(gpt2_tiktoken_bytes, lib)


@pytest.fixture(scope="module")
def vocabs(lib, vocab_bytes, oracle_mod):
    """name -> (device-table vocabulary, oracle vocabulary) for gpt2 / synth100k / synth200k (tests/conftest.py)."""
    cache = {}

    def get(name):
        if name not in cache:
            raw = vocab_bytes(name)
            cache[name] = (N.Vocab(raw, lib), oracle_mod.Vocab(raw))
        return cache[name]
    return get


def test_native_library_is_the_hip_build(lib):
    assert lib.path.endswith(os.path.join("tokenizer_amd", "lib", "libtkz.so"))
    import subprocess
    out = subprocess.run(["strings", "-n", "6", lib.path], capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_golden_gpt2_ids(lib, vocab, lib_rs_bytes):
    exp = load_golden_json("tokens_gpt2.json")
    enc = N.Encoder(vocab, N.P1)
    assert enc.encode_utf8(lib_rs_bytes) == exp                    # TikTokenizerUnitTest.cs:227-245
    enc.set_option(N.OPT_PRETOK_SEQUENTIAL, 1)
    assert enc.encode_utf8(lib_rs_bytes) == exp
    units = np.frombuffer(lib_rs_bytes.decode("utf-8").encode("utf-16-le"), np.uint16).tolist()
    assert enc.encode_utf16(units) == exp


@pytest.mark.parametrize("pattern,sequential", [(1, 0), (2, 0), (3, 0), (4, 0), (1, 1), (2, 1), (3, 1), (4, 1)])
def test_pretok_vs_oracle(lib, vocab, oracle_mod, pattern, sequential):
    parity.check_pretok(lib, oracle_mod, vocab, pattern, sequential, seeds=range(25),
                        kinds=["mix", "ws", "dig", "apo", "oth", "case", "a_ws", "a_dig", "a_apo", "a_oth", "a_mix", "a_brk", "a_case"],
                        doc_lens=[0, 1, 7, 63, 64, 65, 127, 128, 129, 200, 1000, 5000, 9000, 40000], n_docs_choices=(1, 3, 20, 200))


@pytest.mark.parametrize("table", ["builtin", "v8"])
@pytest.mark.parametrize("pattern,sequential", [(1, 0), (2, 0), (3, 0), (1, 1), (2, 1), (3, 1)])
def test_v8_splits(lib, vocab, pattern, sequential, table):
    """The device pre-tokenizers against the pieces of V8, the TypeScript reference's regex engine (tests/v8_cases.py): the whole fixture, packed 1, 3
    and 20 documents to a batch, under the built-in class table and under V8's own."""
    import v8_cases
    v8_cases.check_splits(vocab, pattern, sequential, table, v8_cases.records(pattern, table))


@pytest.mark.parametrize("pattern", [1, 2, 3])
def test_v8_table_read_back(lib, vocab, pattern):
    import v8_cases
    v8_cases.check_table_read_back(vocab, pattern)


@pytest.mark.parametrize("pattern", [1, 2, 3])
def test_v8_table_is_honoured(lib, vocab, pattern):
    import v8_cases
    v8_cases.check_table_is_honoured(vocab, pattern)


def test_v8_one_class_flipped(lib, vocab, oracle_mod):
    import v8_cases
    v8_cases.check_one_class_flipped(vocab, oracle_mod)


@pytest.mark.parametrize("latency_bytes", [None, 0])
@pytest.mark.parametrize("table", ["builtin", "v8"])
@pytest.mark.parametrize("pattern", [1, 2, 3])
def test_v8_ids(lib, vocab, oracle_gpt2, monkeypatch, pattern, table, latency_bytes):
    """encode_batch under the gpt2 table against Encode restated over V8's pieces (whole-piece rank, else the oracle's byte-pair merge): short documents
    one per call (the single launch), then the whole fixture in one batch (the multi-kernel path); again with TKZ_LATENCY_BYTES=0, the form of
    the large batches (test_throughput_setting_on_small_batches)."""
    import v8_cases
    if latency_bytes is not None:
        monkeypatch.setenv("TKZ_LATENCY_BYTES", str(latency_bytes))
    v8_cases.check_ids(vocab, oracle_gpt2, pattern, table, v8_cases.records(pattern, table), single_docs=150 if latency_bytes is None else 10)


@pytest.mark.parametrize("sequential", [0, 1])
def test_hand_derived_splits(lib, vocab, sequential):
    """The device pre-tokenizers against expected pieces written by hand from the regex semantics (tests/hand_splits.py)."""
    from hand_splits import HAND_SPLITS
    encs = {}
    for pat, text, exp in HAND_SPLITS:
        if pat not in encs:
            encs[pat] = N.Encoder(vocab, pat)
            encs[pat].set_option(N.OPT_PRETOK_SEQUENTIAL, sequential)
        b = text.encode("utf-8")
        # once alone, once embedded in a longer ASCII document (the block scanners need full rows to engage)
        # (the separator before the case must not join its first piece: a digit before white space, a newline before anything else)
        sep = b"7" if (text[0].isspace() or text[0] in "\x85\ufeff") else b"\n"
        for pre, post in ((b"", b""), (b"lorem ipsum dolor sit amet " * 12 + sep, b"\n" + b"consectetur adipiscing elit " * 12)):
            doc = pre + b + post
            got = encs[pat].pretokenize(np.frombuffer(doc, np.uint8), np.array([0, len(doc)]))
            starts = [int(i) - len(pre) for i in np.nonzero(got[:len(doc)])[0] if len(pre) <= i < len(pre) + len(b)]
            exp_starts, pos = [], 0
            for piece in exp:
                exp_starts.append(pos)
                pos += len(piece.encode("utf-8"))
            assert starts == exp_starts, (pat, text, bool(pre))


@pytest.mark.parametrize("pattern", [1, 2, 3, 4])
def test_pretok_long_runs(lib, vocab, oracle_mod, pattern):
    # runs that cross rows and whole 4 KiB blocks: the lane scans and the beyond-the-block searches of the block scanners
    parity.check_pretok(lib, oracle_mod, vocab, pattern, 0, seeds=range(12), kinds=("runs",), doc_lens=[3000, 30000, 70000, 300000], n_docs_choices=(1, 3, 9))


@pytest.mark.parametrize("pattern", [N.O200K, N.O200K_DOTNET])
def test_o200k_multibyte_block_scanner(lib, vocab, oracle_mod, pattern):
    blocks, after_ascii, after_mb = parity.check_o200k_blocks(lib, oracle_mod, vocab, ["cjk", "case", "emoji", "upper", "all", "mark", "slash", "chain"], range(12),
                                                              doc_lens=(3000, 9000, 20000, 100000), pattern=pattern)
    assert after_ascii > 0 and after_mb < after_ascii // 5, (blocks, after_ascii, after_mb)
    # `;\n/*` (a '/' swallowed by the tail of a punctuation piece, then more punctuation) and rows of nothing but '/' and line breaks no longer
    # send a block to the sequential matcher: the R4 / ABS flows are iterated and followed through the rows
    b2, a2, m2 = parity.check_o200k_blocks(lib, oracle_mod, vocab, ["mark", "slash"], range(12, 24), pattern=pattern)
    assert a2 > 0 and 10 * m2 < a2, (b2, a2, m2)
    parity.check_o200k_no_sync_points(lib, oracle_mod, vocab, pattern)


def test_host_alloc_buffers(lib, vocab, oracle_mod, oracle_gpt2):
    parity.check_host_alloc(lib, oracle_mod, vocab, oracle_gpt2)


def test_device_unicode_table(lib, vocab):
    parity.check_device_unicode_table(lib, vocab)


def test_golden_splits(lib, vocab):
    # (splits.json: the oracle's, cross-checked against `regex`; splits_o200k_dotnet.json: computed by `regex` on code units, not by the oracle)
    for rec in load_golden_json("splits.json") + load_golden_json("splits_o200k_dotnet.json"):
        enc = N.Encoder(vocab, rec["pattern"])
        b = rec["text"].encode("utf-8")
        got = enc.pretokenize(np.frombuffer(b, np.uint8) if b else np.zeros(0, np.uint8), np.array([0, len(b)]))
        assert [int(i) for i in np.nonzero(got[:len(b)])[0]] == [p[0] for p in rec["pieces"]], rec["text"]


VOCABS = ["gpt2", "synth100k", "synth200k"]


@pytest.mark.parametrize("vname", VOCABS)
def test_every_vocab_key(lib, vocabs, oracle_mod, vname):
    v, ov = vocabs(vname)
    assert len(v) == len(ov) == {"gpt2": 50256, "synth100k": 100256, "synth200k": 199998}[vname]
    parity.check_vocab_keys(lib, oracle_mod, v, ov)


@pytest.mark.parametrize("vname", VOCABS)
def test_pieces_vs_oracle_bpe(lib, vocabs, oracle_mod, vname):
    v, ov = vocabs(vname)
    parity.check_pieces(lib, oracle_mod, v, ov, seed=5, rounds=25 if vname == "gpt2" else 12,
                        lens=[1, 2, 3, 4, 5, 8, 12, 13, 15, 16, 17, 20, 31, 32, 33, 64, 100, 300, 400, 1000, 1023, 1024, 1025, 2048, 3000], counts=[1, 5, 300, 3000])


@pytest.mark.parametrize("vname", ["gpt2", "synth100k", "synth200k"])
def test_piece_memo(lib, vocabs, oracle_mod, vname):
    v, ov = vocabs(vname)
    parity.check_piece_memo(lib, oracle_mod, v, ov)
    parity.check_piece_memo(lib, oracle_mod, v, ov, pattern=N.O200K, seed=31)


@pytest.mark.parametrize("vname,pattern", [("gpt2", N.CL100K), ("synth100k", N.CL100K), ("synth100k", N.P1), ("synth200k", N.O200K_DOTNET)])
def test_promoted_pieces(lib, vocabs, oracle_mod, vname, pattern):
    v, ov = vocabs(vname)
    parity.check_promotion(lib, oracle_mod, v, ov, pattern=pattern)


def test_reserve_takes_allocation_out_of_the_first_call(lib, vocabs, oracle_mod):
    v, ov = vocabs("gpt2")
    parity.check_reserve(lib, oracle_mod, v, ov)


def test_cache_adapts_to_drift(lib, vocabs, oracle_mod, monkeypatch):
    v, ov = vocabs("gpt2")
    parity.check_adaptation(lib, oracle_mod, v, ov, monkeypatch)


def test_memo_is_refreshed_when_full(lib, vocabs, oracle_mod, monkeypatch):
    v, ov = vocabs("gpt2")
    parity.check_memo_refresh(lib, oracle_mod, v, ov, monkeypatch)


def test_host_runtime_defines_the_split(lib, vocabs, oracle_mod):
    v, ov = vocabs("gpt2")
    parity.check_runtime_overrides(lib, oracle_mod, v, ov)


def test_throughput_setting_on_small_batches(lib, vocabs, oracle_mod, monkeypatch):
    """Batches of at most TKZ_OPT_LATENCY_BYTES (16 MB: every batch of this suite) hand missed pieces of more than 32 bytes to k_merge_coop; with the option
    at 0 they are merged a lane each up to 128 bytes, as in the large batches the bench times: the same checks on that setting."""
    monkeypatch.setenv("TKZ_LATENCY_BYTES", "0")
    v, ov = vocabs("gpt2")
    parity.check_miss_lists(lib, oracle_mod, v, ov)
    parity.check_long_pieces_entry_points(lib, oracle_mod, v, ov)
    parity.check_batch(lib, oracle_mod, v, ov, N.CL100K, seed=97, rounds=3, doc_lens=[0, 1, 10, 100, 1000, 6000], n_docs_choices=[1, 4, 40], kinds=("mix", "ws", "oth"))
    # (round 6: the large batches' long misses are binned by length class across the batch and merged off that queue -- k_long_count / k_long_scatter /
    #  k_merge_long_q --: the piece-level checks on that form, trained and adversarial rank tables)
    parity.check_pieces(lib, oracle_mod, v, ov, seed=23, rounds=2, lens=[12, 16, 17, 20, 24, 31, 32, 33, 40, 63, 64, 65, 100, 128, 129, 300], counts=[5, 300, 1200])
    parity.check_pieces(lib, oracle_mod, v, ov, seed=29, rounds=2, lens=[17, 24, 33, 40, 48, 64, 90, 128, 200, 400, 1023, 1024], counts=[40, 400], p_listed=1.0)
    parity.check_random_vocab(lib, oracle_mod, seed=5, n_vocabs=6, lens=[2, 9, 16, 17, 25, 32, 33, 60, 64, 65, 150, 320], n_pieces=60)
    enc = N.Encoder(v, N.CL100K)
    enc.set_option(N.OPT_LATENCY_BYTES, 1 << 20)
    with pytest.raises(N.TkzError):
        enc.set_option(N.OPT_LATENCY_BYTES, -1)


def test_long_pieces_beside_the_short_ones(lib, vocabs, oracle_mod):
    for vname, pat in (("gpt2", N.CL100K), ("synth100k", N.P1)):
        v, ov = vocabs(vname)
        parity.check_side_by_side(lib, oracle_mod, v, ov, pattern=pat)
    v, ov = vocabs("gpt2")
    parity.check_side_by_side_threads(lib, oracle_mod, v, ov)


def test_document_marks(lib, vocabs, oracle_mod):
    v, ov = vocabs("gpt2")
    parity.check_document_marks(lib, oracle_mod, v, ov)


def test_sizing_attempt_and_reused_bitmaps(lib, vocabs, oracle_mod, capfd):
    v, ov = vocabs("gpt2")
    parity.check_sizing_attempt(lib, oracle_mod, v, ov, capfd)


def test_miss_lists(lib, vocabs, oracle_mod):
    for vname, pat, seed in (("gpt2", N.CL100K, 41), ("synth100k", N.CL100K, 44), ("synth200k", N.O200K, 42)):
        v, ov = vocabs(vname)
        parity.check_miss_lists(lib, oracle_mod, v, ov, pattern=pat, seed=seed)
    parity.check_place_paths(lib, oracle_mod)


def test_small_batches_take_one_launch(lib, vocabs, oracle_mod):
    v, ov = vocabs("gpt2")
    parity.check_small_path(lib, oracle_mod, v, ov, rounds=60)
    v, ov = vocabs("synth100k")
    parity.check_small_path(lib, oracle_mod, v, ov, seed=54, rounds=30)


def test_memo_zero_bytes_and_contention(lib, vocabs, oracle_mod):
    """The piece memo under concurrent readers and writers of ONE bucket (two host threads = two streams on one encoder), with NUL-run
    pieces of the contenders' lengths in the same batches; and the rule that pieces holding a zero byte bypass the memo."""
    for vname in ("gpt2", "synth100k"):
        v, ov = vocabs(vname)
        parity.check_memo_zero_bytes(lib, oracle_mod, v, ov)
        parity.check_memo_contention(lib, oracle_mod, v, ov, candidates=400_000, threads=2, rounds=6)


def test_encoder_create_destroy_does_not_leak(lib, vocab):
    """Every encoder owns its tables AND its 16 MB piece memo: creating and destroying encoders must leave the device's free memory flat."""
    import torch
    enc = N.Encoder(vocab, N.CL100K)
    enc.encode_utf8(b"warm up the runtime's own pools")
    enc.close()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(40):
        e = N.Encoder(vocab, N.CL100K)
        e.encode_utf8(b"hello world")
        e.close()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 8 << 20, (free0, free1)          # 40 leaked memos would be 640 MB


@pytest.mark.parametrize("vname", ["gpt2", "synth100k"])
def test_dense_token_region(lib, vocabs, oracle_mod, vname):
    v, ov = vocabs(vname)
    for seed in (17, 18):
        parity.check_dense_region(lib, oracle_mod, v, ov, seed=seed)


def test_mid_pieces_share_the_arena(lib, vocab, oracle_mod, oracle_gpt2):
    # sub-tiles full of 17..1024-byte misses: every pass of the heavy kernel ends on a full arena
    parity.check_pieces(lib, oracle_mod, vocab, oracle_gpt2, seed=11, rounds=12, lens=[17, 24, 33, 40, 48, 64, 90, 128, 200, 400, 1023, 1024], counts=[40, 400, 4000], p_listed=1.0)


@pytest.mark.parametrize("vname", ["gpt2", "synth100k"])
def test_giant_pieces(lib, vocabs, oracle_mod, vname):
    # the 4,000-byte single-letter piece of tokenizer_ts/test/tikTokenizer.test.ts:133, and longer ones
    vocab, oracle_gpt2 = vocabs(vname)
    enc = N.Encoder(vocab, N.CL100K)
    oenc = oracle_mod.Encoder(oracle_gpt2, oracle_mod.CL100K)
    for text in (b"t" * 4000, b"=" * 9000, b" " * 5000 + b"x", b"ab" * 6000, bytes(range(97, 123)) * 400):
        assert enc.encode_utf8(text) == oenc.encode_bytes(text)
    parity.check_long_diverse_pieces(lib, oracle_mod, vocab, oracle_gpt2, lens=(300, 1000, 3000, 9000, 20000, 33000, 50000, 100000))
    parity.check_runs_with_words(lib, oracle_mod, vocab, oracle_gpt2)
    if vname == "gpt2":
        # The last cliff (round-4 review): a piece of more than 32,768 parts used to be brought down to that by rounds in global memory, ONE rank a round --
        # seconds for 100 KB of diverse letters.  Now: sweeps of windows under the local bound (tkz_bpe_window_sweep).  300 KB against the oracle's literal
        # loop (BytePairEncoder.cs:45-64: O(n^2), half a minute on the host), and a bound on the time of the 100 KB piece.
        import random
        import time
        rng = random.Random(77)
        words = [w.decode().strip() for w, _ in oracle_gpt2.entries() if w.strip().isalpha() and len(w.strip()) > 3][:3000]
        big = "".join(rng.choice(words).capitalize() for _ in range(70000))[:300000].encode()
        assert enc.encode_utf8(big) == oenc.encode_bytes(big)
        t100 = big[:100000]
        enc.encode_utf8(t100)
        t0 = time.perf_counter()
        got = enc.encode_utf8(t100)
        ms = (time.perf_counter() - t0) * 1e3
        assert got == oenc.encode_bytes(t100)
        try:       # (the figure DESIGN.md quotes; the directory exists on the GPU box of a gpurun call)
            os.makedirs(os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out"), exist_ok=True)
            with open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out", "giant_100kb_ms.txt"), "w") as f:
                f.write("%.2f ms: one piece of 100,000 bytes of diverse letters, tkz_encode_utf8, second call\n" % ms)
        except OSError:
            pass
        assert ms < 50.0, "100 KB of diverse letters (ONE piece) took %.1f ms" % ms


@pytest.mark.parametrize("pattern,vname", [(1, "gpt2"), (2, "gpt2"), (3, "gpt2"), (4, "gpt2"), (2, "synth100k"), (3, "synth200k"), (4, "synth200k"), (1, "synth200k")])
def test_batch_vs_oracle(lib, vocabs, oracle_mod, pattern, vname):
    v, ov = vocabs(vname)
    parity.check_batch(lib, oracle_mod, v, ov, pattern, seed=11 + pattern, rounds=12 if vname == "gpt2" else 8,
                       doc_lens=[0, 1, 10, 100, 1000, 6000, 30000], n_docs_choices=[1, 4, 40, 400], kinds=("mix", "ws", "oth", "dig", "apo", "case", "a_mix", "a_brk", "a_ws", "a_dig"))


@pytest.mark.parametrize("vname", ["gpt2", "synth100k"])
def test_decode_round_trip(lib, vocabs, oracle_mod, vname):
    v, ov = vocabs(vname)
    parity.check_decode(lib, oracle_mod, v, ov, rounds=10)


def test_decode_sparse_rank_table(lib, oracle_mod):
    # ranks up to ~2^26: the decoder table takes its sorted (binary-search) form
    import random
    raw = parity.random_vocab_bytes(random.Random(4), alphabet=b"abc", n_keys=200, rank_step=97_003, rank_base=4_200_000)
    parity.check_decode(lib, oracle_mod, N.Vocab(raw, lib), oracle_mod.Vocab(raw), rounds=2)


@pytest.mark.parametrize("pattern", [1, 2, 3, 4])
def test_piece_granular_batch(lib, vocab, oracle_mod, oracle_gpt2, pattern):
    parity.check_piece_granular(lib, oracle_mod, vocab, oracle_gpt2, pattern, rounds=20)


def test_shard_writer_c_abi(lib, tmp_path):
    """tkz_shard_write / tkz_shard_write_device / tkz_shard_read_header against the memory-mapping reader."""
    from tokenizer_amd import Shard
    rng = np.random.default_rng(5)
    n_docs = 3_000_000                                     # 24 MB of offsets + ~230 MB of ids: several 32 MiB chunks
    counts = rng.integers(0, 40, n_docs)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ids = rng.integers(0, 200_000, int(offs[-1])).astype(np.int32)
    p = str(tmp_path / "h.tkzs")
    N.shard_write(p, ids, offs, 77, 1234, lib=lib)
    assert N.shard_read_header(p, lib=lib) == (n_docs, len(ids), 77, 1234)
    sh = Shard(p)
    assert np.array_equal(np.asarray(sh.ids), ids) and np.array_equal(np.asarray(sh.offsets), offs) and (sh.doc_base, sh.token_base) == (77, 1234)
    with pytest.raises(N.TkzError):
        N.shard_write(p, ids, offs[::-1].copy(), lib=lib)
    import torch
    d_ids, d_offs = torch.from_numpy(ids).cuda(), torch.from_numpy(offs).cuda()
    p2 = str(tmp_path / "d.tkzs")
    N.shard_write_device(p2, d_ids.data_ptr(), len(ids), d_offs.data_ptr(), n_docs, 77, 1234, device=0, lib=lib)
    assert open(p2, "rb").read() == open(p, "rb").read()


def test_errors_and_edges(lib, vocab, oracle_mod):
    parity.check_errors(lib, oracle_mod, vocab)


def test_utf16_entry(lib, vocab, oracle_mod, oracle_gpt2):
    parity.check_utf16(lib, oracle_mod, vocab, oracle_gpt2)


def test_utf16_batch_entry(lib, vocab, oracle_mod, oracle_gpt2):
    parity.check_utf16_batch(lib, oracle_mod, vocab, oracle_gpt2, **dict(rounds=12, doc_counts=(1, 7, 60, 600), max_units=2500))


# ---- device-resident path at scale ------------------------------------------------------------------

def _device_run(lib, vocab, kind, pattern, n_docs, lo, hi, seed, sequential=False, first_doc=0):
    import torch
    dev = torch.device("cuda", 0)
    enc = N.Encoder(vocab, pattern)
    if sequential:
        enc.set_option(N.OPT_PRETOK_SEQUENTIAL, 1)
    st = torch.cuda.current_stream().cuda_stream
    d_offs = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    total = N.corpus_generate_device(0, kind, seed, first_doc, n_docs, lo, hi, d_offs.data_ptr(), None, 0, st, lib=lib)
    d_bytes = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    N.corpus_generate_device(0, kind, seed, first_doc, n_docs, lo, hi, d_offs.data_ptr(), d_bytes.data_ptr(), total, st, lib=lib)
    d_ids = torch.empty(total, dtype=torch.int32, device=dev)
    d_ooffs = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    ntok = enc.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, total, d_ids.data_ptr(), total, d_ooffs.data_ptr(), st)
    return dict(enc=enc, total=total, ntok=ntok, d_offs=d_offs, d_bytes=d_bytes, d_ids=d_ids[:ntok], d_ooffs=d_ooffs)


def _token_lengths(ovocab):
    ents = ovocab.entries()
    tl = np.zeros(max(r for _, r in ents) + 1, np.int64)
    for k, r in ents:
        tl[r] = len(k)
    return tl


@pytest.mark.parametrize("vname,kind,pattern,n_docs,lo,hi", [
    ("gpt2", 1, 2, 400_000, 256, 768), ("synth100k", 1, 2, 400_000, 256, 768), ("synth100k", 2, 2, 200_000, 256, 768),
    ("synth200k", 3, 3, 1_500, 30_000, 34_000), ("gpt2", 1, 1, 100_000, 16, 128), ("synth100k", 3, 2, 1_500, 30_000, 34_000),
    ("synth200k", 2, 3, 100_000, 256, 768), ("synth200k", 2, 4, 100_000, 256, 768),
    # BASELINE.json configs[1], [2] and one GPU's share of [4] at full size, on the stand-ins of the vocabularies they name
    ("synth100k", 1, 2, 10_000_000, 256, 768), ("synth100k", 2, 2, 2_000_000, 256, 768), ("synth200k", 3, 3, 32_768, 30_000, 34_000),
    # one GPU's share of BASELINE.json configs[3] (100 M documents over 8 GPUs): the LAST rank's 12.5 M documents
    ("synth100k", 1, 2, 12_500_000, 256, 768)])
def test_device_corpus_properties_and_sample(lib, vocabs, oracle_mod, vname, kind, pattern, n_docs, lo, hi):
    import torch
    vocab, oracle_gpt2 = vocabs(vname)
    first_doc = 7 * n_docs if n_docs == 12_500_000 else 0
    r = _device_run(lib, vocab, kind, pattern, n_docs, lo, hi, 0x5EED0000 + kind, first_doc=first_doc)
    ooffs = r["d_ooffs"]
    assert int(ooffs[0]) == 0 and int(ooffs[-1]) == r["ntok"]
    counts = ooffs[1:] - ooffs[:-1]
    doc_len = r["d_offs"][1:] - r["d_offs"][:-1]
    assert bool((counts >= 0).all()) and bool((counts <= doc_len).all())
    # property over EVERY document: the byte lengths of a document's tokens add up to the document (decode length)
    tl = torch.from_numpy(_token_lengths(oracle_gpt2)).to(ooffs.device)
    ids = r["d_ids"].long()
    assert int(ids.min()) >= 0 and int(ids.max()) < len(tl)
    csum = torch.zeros(r["ntok"] + 1, dtype=torch.int64, device=ooffs.device)
    csum[1:] = torch.cumsum(tl[ids], 0)
    assert bool(((csum[ooffs[1:]] - csum[ooffs[:-1]]) == doc_len).all())
    # decode(encode(x)) == x for the WHOLE batch, on the device (TikTokenizer.Decode, TikTokenizer.cs:586-604; the round trip
    # every reference test asserts, TikTokenizerUnitTest.cs:47-48): bytes and document offsets
    d_back = torch.empty(r["total"] + 64, dtype=torch.uint8, device=ooffs.device)
    d_boffs = torch.empty(n_docs + 1, dtype=torch.int64, device=ooffs.device)
    nb = r["enc"].decode_batch_device(r["d_ids"].data_ptr(), ooffs.data_ptr(), n_docs, r["ntok"], d_back.data_ptr(), r["total"], d_boffs.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    assert nb == r["total"] and torch.equal(d_back[:nb], r["d_bytes"][:nb]) and torch.equal(d_boffs, r["d_offs"])
    del d_back, d_boffs
    # bit-exact vs the oracle on EVERY document of the batch, on all host cores (tkzo_check_batch: each document is encoded and
    # compared in place with the ids the GPU left for it -- 10 M documents / 5.1 GB take a few seconds and no extra memory)
    h_offs = r["d_offs"].cpu().numpy()
    h_ooffs = ooffs.cpu().numpy()
    h_ids = r["d_ids"].cpu().numpy()
    h_bytes = r["d_bytes"][:r["total"]].cpu().numpy()
    bad, first_bad, otok = oracle_mod.check_batch(oracle_gpt2, pattern, h_bytes, h_offs, h_ids, h_ooffs, threads=max(1, os.cpu_count() or 1))
    assert (bad, first_bad, otok) == (0, -1, r["ntok"]), "%d of %d documents differ from the oracle, first %d" % (bad, n_docs, first_bad)
    # the generator: device == host, on a stride of documents
    pick = sorted(set(list(range(0, min(n_docs, 300))) + list(range(0, n_docs, max(1, n_docs // 300))) + [n_docs - 1]))
    for d in pick:
        doc = h_bytes[h_offs[d]:h_offs[d + 1]].tobytes()
        assert doc == N.corpus_doc_host(kind, 0x5EED0000 + kind, d + first_doc, lo, hi, lib=lib)


def test_utf16_document_spanning_chunk_cuts(lib, vocabs, oracle_mod):
    """tkz_encode_batch_utf16 with ONE document of 7 M code units (14 MB: the batch is cut into two chunks on document boundaries, so one chunk holds the
    document and the other nothing at all) -- alone, last and first in its batch.  Round 5's advisor: the empty chunk launched k_u16_len / the scan on a grid
    of 0 workgroups, which HIP refuses."""
    import random
    import regex_crosscheck as RC
    vocab, ov = vocabs("gpt2")
    enc = N.Encoder(vocab, N.CL100K)
    oenc = oracle_mod.Encoder(ov, N.CL100K)
    rng = random.Random(5)
    alpha = RC.alphabet()
    piece = RC.to_units(RC.random_text(rng, alpha, 70_000))
    long_doc = (piece * (7_000_000 // len(piece) + 1))[:7_000_000]
    if 0xD800 <= long_doc[-1] < 0xDC00: long_doc[-1] = 0x41                        # (no lone half at the cut of the tiling)
    want_long = oenc.encode_utf16(long_doc)
    small = [RC.to_units(RC.random_text(rng, alpha, rng.randint(0, 200))) for _ in range(5)]
    for docs in ([long_doc], small + [long_doc], [long_doc] + small, [[]] * 2 + [long_doc] + [[]] * 2):
        flat = np.concatenate([np.asarray(d, dtype=np.uint16) for d in docs]) if docs else np.zeros(0, np.uint16)
        offs = np.cumsum([0] + [len(d) for d in docs]).astype(np.int64)
        ids, ooff = enc.encode_batch_utf16(flat, offs)
        for d, units in enumerate(docs):
            got = ids[ooff[d]:ooff[d + 1]].tolist()
            assert got == (want_long if units is long_doc else oenc.encode_utf16(units)), (len(docs), d)


def test_host_path_chunked_and_threads(lib, vocabs, oracle_mod):
    """tkz_encode_batch_utf8 on host buffers at a size that is cut into chunks (upload k+1 / kernels k / download k-1 overlapped),
    pageable and page-locked, against the device-resident path; then two host threads on ONE encoder at the same time (each call
    leases its own workspace and streams): both get the right answer."""
    import threading
    import time
    import torch
    vocab, ov = vocabs("synth100k")
    n, lo, hi, seed = 600_000, 256, 768, 0x5EED0002
    r = _device_run(lib, vocab, 1, 2, n, lo, hi, seed)
    h_bytes = r["d_bytes"][:r["total"]].cpu().numpy()
    h_offs = r["d_offs"].cpu().numpy()
    want_ids, want_offs = r["d_ids"].cpu().numpy(), r["d_ooffs"].cpu().numpy()
    enc = r["enc"]
    ids, ooff = enc.encode_batch(h_bytes, h_offs)                                  # pageable buffers
    assert np.array_equal(ids, want_ids) and np.array_equal(ooff, want_offs)
    pb = torch.from_numpy(h_bytes).pin_memory()
    po = torch.from_numpy(h_offs).pin_memory()
    out = (torch.zeros(len(h_bytes), dtype=torch.int32).pin_memory().numpy(), torch.zeros(n + 1, dtype=torch.int64).pin_memory().numpy())
    t0 = time.perf_counter()
    ids, ooff = enc.encode_batch(pb.numpy(), po.numpy(), out=out)                  # page-locked buffers: fully asynchronous copies
    dt = time.perf_counter() - t0
    assert np.array_equal(ids, want_ids) and np.array_equal(ooff, want_offs)
    print("host path, page-locked buffers: %.1f GB/s" % (len(h_bytes) / dt / 1e9))
    # the chunks' results left on a copy engine of their own (csrc/tkz_sdma.cpp): ids + offsets of every chunk -- unless the run switched that off
    # (where the HSA runtime under HIP has the entry point at all: the path is optional by design, csrc/tkz_sdma.h)
    import ctypes
    try:
        has_engine_copy = hasattr(ctypes.CDLL("libhsa-runtime64.so.1"), "hsa_amd_memory_async_copy_on_engine")
    except OSError:
        has_engine_copy = False
    if os.environ.get("TKZ_D2H_ENGINE") != "-1" and has_engine_copy:
        assert enc.engine_downloads >= 2 * (len(h_bytes) // (24 << 20)), enc.engine_downloads
    # mid-size page-locked batches: 20 MB (chunks of a quarter of the batch), 3 MB (one chunk, fetched by k_ingest, ids
    # written by k_place itself) -- twice each: a fresh workspace, then a sized one
    for nd in (40_000, 6_000):
        cb = int(h_offs[nd]); nt = int(want_offs[nd])
        for _ in range(2):
            out[0][:] = -1
            ids, ooff = enc.encode_batch(pb.numpy()[:cb], po.numpy()[:nd + 1], out=(out[0][:cb], out[1][:nd + 1]))
            assert np.array_equal(ids, want_ids[:nt]) and np.array_equal(ooff, want_offs[:nd + 1]), nd
    # two threads, two different batches, one encoder
    half = n // 2
    cutb = int(h_offs[half])
    parts = [(h_bytes[:cutb], h_offs[:half + 1]), (h_bytes[cutb:], h_offs[half:] - cutb)]
    res = [None, None]

    def work(i):
        for _ in range(3):
            res[i] = enc.encode_batch(parts[i][0], parts[i][1])
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    ntok0 = int(want_offs[half])
    assert np.array_equal(res[0][0], want_ids[:ntok0]) and np.array_equal(res[0][1], want_offs[:half + 1])
    assert np.array_equal(res[1][0], want_ids[ntok0:]) and np.array_equal(res[1][1], want_offs[half:] - ntok0)


def test_rccl_communicator_counts(lib, vocab):
    """The C ABI's direct-RCCL communicator (tkz_comm_*): RCCL is initialised through libtkz and the count all-gather runs both
    asynchronously on the encode stream (table kept in HBM) and in its blocking host form.  world = 1 on a one-GPU box (RCCL
    admits one rank per device); the N-rank arithmetic is covered by test_eight_shards_on_one_device."""
    import torch
    from tokenizer_amd import sharded
    c = sharded.RcclCounts(0, 1, 0, lambda b: b, lib=lib)
    info = c.info()
    assert info["world_size"] == 1 and info["rank"] == 0 and info["backend"].startswith("rccl ")
    r = _device_run(lib, vocab, 1, 2, 50_000, 256, 768, 0x5EED0002)
    st = torch.cuda.current_stream().cuda_stream
    c.gather_async(r["enc"], st)
    g = c.result()
    assert g["table"].tolist() == [[50_000, r["total"], r["ntok"]]] and (g["doc_base"], g["token_base"]) == (0, 0)
    assert (g["docs"], g["bytes"], g["tokens"]) == (50_000, r["total"], r["ntok"])
    g2 = c.gather(7, 8, 9)
    assert g2["table"].tolist() == [[7, 8, 9]]
    c.close()


def test_eight_shards_on_one_device(lib, vocabs):
    """BASELINE configs[3]'s partitioning with the 8 ranks faked on one device: rank r encodes documents tkz_shard_range(r) of the
    job; the per-rank counts form the table the all-gather would deliver; tkz_shard_bases gives every rank its global bases; the
    shards laid out at those bases reproduce the single-batch result exactly (ids and document offsets)."""
    import torch
    vocab, _ = vocabs("synth100k")
    n, lo, hi, seed, world = 400_000, 256, 768, 0x5EED0002, 8
    whole = _device_run(lib, vocab, 1, 2, n, lo, hi, seed)
    parts, table = [], []
    for r in range(world):
        a, b = N.shard_range(n, r, world, lib=lib)
        assert (a, b) == ((n * r) // world, (n * (r + 1)) // world)
        p = _device_run(lib, vocab, 1, 2, b - a, lo, hi, seed, first_doc=a)
        parts.append(p)
        table.append([b - a, p["total"], p["ntok"]])
    ids = torch.empty_like(whole["d_ids"])
    ooffs = torch.empty_like(whole["d_ooffs"])
    for r, p in enumerate(parts):
        bases, totals = N.shard_bases(table, r, lib=lib)
        assert totals == [n, whole["total"], whole["ntok"]]
        ids[bases[2]:bases[2] + p["ntok"]] = p["d_ids"]
        ooffs[bases[0]:bases[0] + table[r][0] + 1] = p["d_ooffs"] + bases[2]
    assert torch.equal(ids, whole["d_ids"]) and torch.equal(ooffs, whole["d_ooffs"])


def test_shard_invariance(lib, vocab):
    """ids of a batch == ids of its two halves encoded separately (documents are independent)."""
    import torch
    n, lo, hi, seed = 60_000, 256, 768, 0x5EED0002
    whole = _device_run(lib, vocab, 1, 2, n, lo, hi, seed)
    a = _device_run(lib, vocab, 1, 2, n // 2, lo, hi, seed, first_doc=0)
    b = _device_run(lib, vocab, 1, 2, n - n // 2, lo, hi, seed, first_doc=n // 2)
    assert whole["ntok"] == a["ntok"] + b["ntok"]
    assert torch.equal(whole["d_ids"], torch.cat([a["d_ids"], b["d_ids"]]))
    assert torch.equal(whole["d_ooffs"], torch.cat([a["d_ooffs"], b["d_ooffs"][1:] + a["ntok"]]))


@pytest.mark.parametrize("kind,pattern", [(1, 2), (2, 2), (3, 2), (2, 1)])
def test_parallel_and_sequential_pretok_agree_at_scale(lib, vocab, kind, pattern):
    import torch
    lo, hi, n = (30_000, 34_000, 600) if kind == 3 else (256, 768, 100_000)
    p = _device_run(lib, vocab, kind, pattern, n, lo, hi, 0x5EED0000 + kind)
    s = _device_run(lib, vocab, kind, pattern, n, lo, hi, 0x5EED0000 + kind, sequential=True)
    assert p["ntok"] == s["ntok"] and torch.equal(p["d_ids"], s["d_ids"]) and torch.equal(p["d_ooffs"], s["d_ooffs"])


def test_reference_unit_tests_restated(lib, gpt2_tiktoken_bytes, lib_rs_bytes, oracle_mod, oracle_gpt2):
    import reference_style
    reference_style.run_gpt2_suite(lib, gpt2_tiktoken_bytes, lib_rs_bytes.decode("utf-8"), oracle_mod, oracle_gpt2)
    reference_style.run_cl100k_suite(lib)      # runs only when cl100k_base.tiktoken is supplied


def test_mirror_takes_the_hosts_runtime(lib, gpt2_tiktoken_bytes, oracle_mod, oracle_gpt2):
    import reference_style
    reference_style.run_host_runtime_suite(lib, gpt2_tiktoken_bytes, oracle_mod, oracle_gpt2)


def test_builders_by_name_pick_the_defining_engine(lib, vocab_bytes, oracle_mod, tmp_path):
    import reference_style
    reference_style.run_by_name_suite(lib, vocab_bytes, oracle_mod, tmp_path)


def test_adversarial_rank_tables(lib, oracle_mod):
    parity.check_random_vocab(lib, oracle_mod, seed=3, n_vocabs=40, lens=[2, 5, 9, 16, 17, 25, 32, 33, 60, 150, 320, 1024, 1025, 3000], n_pieces=200)
    # arbitrary rank tables on pieces that start in the global pool and end in the tail that keeps only the pair ranks in LDS
    parity.check_random_vocab(lib, oracle_mod, seed=4, n_vocabs=6, lens=[17000, 20000, 30000, 33000], n_pieces=4)
    # ... with keys of up to 300 bytes (the local bound of the tail's proposals, a window of ten blocks) and of up to 1100 (the global bound)
    parity.check_random_vocab(lib, oracle_mod, seed=5, n_vocabs=6, lens=[300, 777, 1024, 3000, 18000, 33000], n_pieces=6, max_len=300)
    parity.check_random_vocab(lib, oracle_mod, seed=6, n_vocabs=4, lens=[300, 1024, 3000, 18000], n_pieces=6, max_len=1100)


@pytest.mark.parametrize("vname", ["gpt2", "synth100k"])
def test_long_pieces_through_every_entry_point(lib, vocabs, oracle_mod, vname):
    v, ov = vocabs(vname)
    for seed in (13, 14, 15):
        parity.check_long_pieces_entry_points(lib, oracle_mod, v, ov, seed=seed)


def test_device_entry_in_two_halves(lib, vocabs, oracle_mod):
    """tkz_encode_batch_device_begin / _end with four batches in flight on two streams."""
    import torch
    dev = torch.device("cuda", 0)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def upload(a):
        tns = torch.from_numpy(a).to(dev)
        return tns, tns.data_ptr()
    torch.cuda.synchronize()
    for vname in ("gpt2", "synth100k"):
        v, ov = vocabs(vname)
        parity.check_begin_end(lib, oracle_mod, v, ov, upload=upload, streams=(s1.cuda_stream, s2.cuda_stream))
