"""`not gpu`: token-budget buckets (tkz_encode_batch_budgeted_device / _utf8 / _utf16; k_tbk_mark, k_tbk_chain, k_tbk_table, k_tbk_write) -- the real kernel
sources on the CPU emulator (tests/hostemu/), exact against the rule of tkz.h restated as the sequential greedy loop over the oracle's ids
(tests/budgeted_cases.py).  tests/test_gpu_budgeted.py runs the same cases on the hardware, on gpt2 and on synth100k."""
import os
import re

import pytest

import budgeted_cases as TB
import emu
from conftest import ROOT
from tokenizer_amd import _native as N


@pytest.fixture(scope="module")
def lib():
    return emu.library()


@pytest.fixture(scope="module")
def raw(vocab_bytes):
    return vocab_bytes("gpt2")


@pytest.fixture(scope="module")
def make(lib, oracle_mod, raw):
    def make_ctx(specials=None, pattern=N.CL100K, options=(), vocab=None):
        return TB.Ctx(lib, oracle_mod, vocab or raw, pattern, specials, options=options)
    return make_ctx


@pytest.fixture(scope="module")
def ctx(make):
    return make()


def test_the_kernel_text():
    src = os.path.join(ROOT, "tokenizer_amd", "csrc")
    text = open(os.path.join(src, "tkz_kernels.hip")).read()
    head = open(os.path.join(src, "tkz_kernels.h")).read()
    assert re.search(r"\bkTbkMarkTile = %d\b" % TB.T_MARK, head) and re.search(r"\bkTbkLook = %d\b" % TB.LOOK, head) and TB.T_MARK % 64 == 0 and TB.LOOK == 64
    # a banner section of its own between the launchers and the bucketed section, which stays where it was
    first, end = text.index("// Token-budget buckets (tkz_encode_batch_budgeted_device"), text.index("// Length-bucketed padded rows (tkz_encode_batch_bucketed_device")
    assert text.index("void launch_corpus(") < first < end and text.count("// Token-budget buckets (tkz_encode_batch_budgeted_device") == 1
    body = text[first:end]
    # plain C++ and the helpers of tkz_simt.h; nothing is added up in memory and nothing depends on timing
    assert "asm" not in body and "atomic" not in body and "fence" not in body and "__builtin" not in body and "rocprim" not in body and "hipcub" not in body
    assert body.count("TKZ_KERNEL(256) void k_tbk_") == 4 and "simt::ballot(" in body and "simt::sync()" not in body
    for reused in ("TKZ_KERNEL(256) void k_pad_lens(PadParams K);", "TKZ_KERNEL(256) void k_bkt_hist(BktParams K,", "TKZ_KERNEL(256) void k_bkt_scatter(BktParams K,"):
        assert reused in body                                    # the bucketed call's kernels are reused as they are: declared here, defined in their own sections
    # the only sequential stage: ONE workgroup of one wavefront, and no loop over the buckets in it
    assert body.count("TKZ_LAUNCH(k_tbk_chain, 1, 64, L.stream, K);") == 1 and body.count("TKZ_LAUNCH(k_tbk_chain") == 1
    chain = body[body.index("void k_tbk_chain("):body.index("void k_tbk_table(")]
    assert "while (s < n && j < nruns)" in chain and chain.count("tkz_tbk_ahead(") == 2 and "for (" not in chain
    write = body[body.index("void k_tbk_write("):body.index("int64_t tbk_run_cap(")]
    assert "tkz_load_nt(" in write and write.count("tkz_store_nt(") == 3 and write.count("tkz_last_le(") == 1      # one search a tile, none a lane
    assert write.count(" / ") == 4 and write.count("kThreads / 64") == 2 and write.count(" / (int64_t)s.W") == 1 and " % " not in write      # nothing is divided per position
    assert write.index("tkz_load_nt(") < write.index("tkz_store_nt(")      # the next group's loads are requested before this group's stores
    assert "K.bucket_cap" in write and "Q.out_cap" in write             # both capacity checks on the device
    step = body[body.index("void tkz_tbk_step("):body.index("void k_tbk_write(")]
    assert step.count(" / s.W") == 1 and step.count(" % s.W") == 1


def test_the_header_states_the_rule():
    text = open(os.path.join(ROOT, "include", "tkz.h")).read()
    block = text[text.index("/* ---- Token-budget buckets"):text.index("void tkz_encoder_budgeted_calls(")]
    for needle in ("THE RULE", "1 <= B <= 2^31 - 1, and 2^31 - 1 means none", "max_len <= T <= 2^62", "bucket_cap >= 0", "EXACTLY as in the bucketed rule", "w(0) = 0",
                   "w(l) = min(L, ceil(l / M) * M)", "Bucket 0 starts at sorted row 0", "largest e in (s, n_docs] with e - s <= B", "<= T", "row e - 1 ascending and of row s descending",
                   "only B stops them", "the last entry is n_docs", "the last entry is P", "out[bucket_offsets[b] + i * W_b .. + W_b)", "*n_buckets",
                   "n_buckets = 2; rows 0, 3, 5; widths 3, 4; bucket offsets 0, 9, 17", "X P P / c1 c2 X / e1 e2 X | a1 a2 a3 X / d1 d2 d3 X",
                   "n_buckets = 2; rows 0, 2, 5; widths 4, 3; bucket offsets 0, 8, 17", "a1 a2 a3 X / d1 d2 d3 X | c1 c2 X / e1 e2 X / X P P",
                   "rows 0, 2, 4, 5; widths 3, 4, 4; bucket offsets 0, 6, 14, 18", "bucket_rows_out[b] = min(b * B, n_docs)",
                   "TKZ_E_CAPACITY when out_cap < P or bucket_cap < n_buckets", "All four scalars", "n_docs * L positions and n_docs buckets ALWAYS suffice",
                   "NEVER the uncut ids", "Known limit", "required_batch_size_multiple", "no shuffling", "no maximum per document", "UNPADDED tokens", "_begin / _end",
                   "no chunk pipeline", "no device-resident UTF-16"):
        assert needle in block, needle
    bucketed = text[text.index("/* ---- Length-bucketed padded rows"):text.index("void tkz_encoder_bucketed_calls(")]
    assert "the budgeted entries below" in bucketed               # the bucketed block's last paragraph points here


def test_the_worked_examples(ctx):
    TB.check_worked_examples(ctx)


def test_one_run_many_buckets(ctx):
    TB.check_one_run(ctx)


def test_runs_ascending(ctx):
    TB.check_runs(ctx, TB.ASC)


def test_runs_descending(ctx):
    TB.check_runs(ctx, TB.DESC)


def test_width_zero(ctx):
    TB.check_width_zero(ctx)


def test_run_counts_at_the_chain_geometry(ctx):
    TB.check_run_counts(ctx)


def test_documents_around_the_tiles(ctx):
    TB.check_tiles(ctx)


def test_more_documents_than_the_grids_hold(ctx, lib):
    TB.check_grid_stride(ctx, lib)


def test_only_the_row_cap_binds(ctx):
    TB.check_row_cap_only(ctx)


def test_random_batches_against_the_greedy_loop(ctx):
    TB.check_random(ctx)


def test_special_tokens(make):
    TB.check_special(make)


def test_capacity_and_argument_errors(make):
    TB.check_capacity(make)


def test_agreement_of_the_entries(make, lib):
    TB.check_agreement(make, lib)


def test_an_attempt_run_again(make):
    TB.check_retry(make)


def test_python_mirror(lib, oracle_mod, raw, lib_rs_bytes):
    TB.check_python_mirror(lib, oracle_mod, raw, lib_rs_bytes.decode("utf-8"))
