"""`not gpu`: the frame of tkz_probe_subtile -- text request, bitmap words, the end of the last piece, record stores, the pre-pass's keys
(tests/probe_frame_cases.py) -- the real kernel sources on the CPU emulator (tests/hostemu/), ids and offsets against the oracle.  Every case runs as a batch
small enough for the single launch (k_small) and padded past it (k_probe; the special case: k_probe_special).  tests/test_gpu_probe_frame.py runs the same
cases on the hardware."""
import os
import re

import pytest

import emu
import probe_frame_cases as PC
from conftest import ROOT
from tokenizer_amd import _native as N

PADDED = pytest.mark.parametrize("padded", [False, True], ids=["k_small", "batch"])
TABLES = pytest.mark.parametrize("table", ["gpt2", "synth100k"])


@pytest.fixture(scope="module")
def ctxs(oracle_mod, vocab_bytes):
    made = {}

    def get(table, special=False):
        if (table, special) not in made:
            made[table, special] = PC.Ctx(emu.library(), oracle_mod, vocab_bytes(table), N.CL100K, PC.SC.SPECIAL_SETS[table] if special else None)
        return made[table, special]
    return get


def test_the_kernel_text():
    src = os.path.join(ROOT, "tokenizer_amd", "csrc")
    text = open(os.path.join(src, "tkz_kernels.hip")).read()
    header = open(os.path.join(src, "tkz_kernels.h")).read()
    tables = open(os.path.join(src, "tkz_tables.h")).read()
    assert re.search(r"\bkSub = %d\b" % PC.SUB, header) and re.search(r"\bkHalo = %d\b" % PC.HALO, header)
    assert re.search(r"#define TKZ_SHORT_KEY_MAX %d\b" % (PC.MID_MIN - 1), tables) and re.search(r"#define TKZ_MID_KEY_MAX %d\b" % PC.MID_MAX, tables)
    # (what check_record_capacity's 48 KB of one-byte pieces exceed: a fresh workspace's record per three bytes)
    assert re.search(r"total\s*/\s*3\s*\+\s*8\s*\*\s*ntiles\s*\+\s*4096", open(os.path.join(src, "tkz_api.cpp")).read())
    # a mask row per key length up to the longest key of the pre-pass (check_mid_keys runs every one of them)
    assert re.search(r"\bkProbeMaskRows\s*=\s*TKZ_MID_KEY_MAX\s*\+\s*1\b", text)


@TABLES
@PADDED
def test_totals(ctxs, table, padded):
    PC.check_totals(ctxs(table), padded)


@TABLES
@PADDED
def test_last_piece(ctxs, table, padded):
    PC.check_last_piece(ctxs(table), padded)


@TABLES
@PADDED
def test_long_runs(ctxs, table, padded):
    PC.check_long_runs(ctxs(table), padded)


@TABLES
@PADDED
def test_edge_starts(ctxs, table, padded):
    PC.check_edge_starts(ctxs(table), padded)


@TABLES
@PADDED
def test_document_marks(ctxs, table, padded):
    PC.check_document_marks(ctxs(table), padded)


@TABLES
@PADDED
def test_mid_keys(ctxs, table, padded):
    PC.check_mid_keys(ctxs(table), padded)


@TABLES
@PADDED
def test_halo_edge(ctxs, table, padded):
    PC.check_halo_edge(ctxs(table), padded)


@TABLES
@PADDED
def test_record_capacity(ctxs, table, padded):
    PC.check_record_capacity(ctxs(table), padded)


@TABLES
@PADDED
def test_special(ctxs, table, padded):
    PC.check_special(ctxs(table, True), padded)
