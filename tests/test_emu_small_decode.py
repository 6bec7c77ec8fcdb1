"""`not gpu`: Decode(int[]) for one id list in a single launch (tkz_decode_utf8 / _utf16, k_dec_small) -- the real kernel sources on the CPU emulator
(tests/hostemu/), exact against the vocabulary's keys, the plain UTF-8 reference of tests/u8_decode_cases.py and the batch entries.
tests/test_gpu_small_decode.py runs the same cases on the hardware, every one on both tables."""
import os
import re

import pytest

import emu
import small_decode_cases as SD
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    return emu.library()


@pytest.fixture(scope="module")
def dec(lib, vocab_bytes, oracle_mod):
    cache = {}

    def get(table):
        if table not in cache:
            cache[table] = SD.setup(lib, vocab_bytes("gpt2"), oracle_mod, table)
        return cache[table]
    return get


def test_constants_are_the_kernels():
    src = os.path.join(ROOT, "tokenizer_amd", "csrc")
    text = open(os.path.join(src, "tkz_kernels.h")).read() + open(os.path.join(src, "tkz_kernels.hip")).read()

    def const(name):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
        assert m, name
        return int(m.group(1))
    assert (const("kDecSmallMaxIds"), const("kDecSmallMaxBytes"), const("kDecSmallStage"), const("kDecSmallWaves")) == (SD.MAX_IDS, SD.MAX_BYTES, SD.STAGE, SD.WAVES)
    assert const("kDecTile") == const("kU8Tile") == SD.TILE
    assert re.search(r"A\.n_ids <= %d \* kDecTile \? 256 : 1024" % SD.WAVES_SMALL, text)
    # the route threshold is the capacity (profiles/small_decode/README.md)
    assert re.search(r"#define TKZ_SMALL_DECODE_MAX_IDS %d\b" % SD.MAX_IDS, text)
    # one workgroup, barriers only: the kernel holds no atomic and no fence
    body = text[text.index("void k_dec_small("):text.index("// launchers")]
    assert "atomic" not in body and "fence" not in body and body.count("simt::sync()") == 1 and body.count("tkz_dec_small_scan(") == 2


def test_the_tables(dec):
    enc, S = dec("dense")
    assert enc.small_decode_calls() == (0, 0) and len(S.key_of[S.longest]) * SD.TILE == SD.MAX_BYTES        # (gpt2: 128 bytes)
    _, S2 = dec("sparse")
    assert max(S2.specials.values()) >= 1 << 22 and "\U0001F600" in SD.FAR_LITERAL


@pytest.mark.parametrize("table", SD.TABLES)
def test_id_totals(dec, table):
    SD.check_id_totals(*dec(table))


@pytest.mark.parametrize("table", SD.TABLES)
def test_byte_tile_edges(dec, table):
    SD.check_byte_edges(*dec(table))


@pytest.mark.parametrize("table", SD.TABLES)
def test_stage_overflow_and_capacity_edges(dec, table):
    SD.check_stage_and_capacity(*dec(table))


@pytest.mark.parametrize("table", SD.TABLES)
def test_ids_outside_the_vocabulary(dec, table):
    SD.check_outside_ids(*dec(table))


def test_arguments(dec):
    SD.check_arguments(*dec("dense"))


@pytest.mark.parametrize("table", SD.TABLES)
def test_capacity_on_every_route(dec, table):
    SD.check_capacity(*dec(table))


@pytest.mark.parametrize("table", SD.TABLES)
def test_agreement_with_the_batch_entries(dec, table):
    SD.check_agreement(*dec(table))


def test_reuse_and_interleaved_encode_calls(dec):
    SD.check_reuse(*dec("dense"))


def test_two_threads_share_one_encoder(dec):
    SD.check_threads(*dec("sparse"))


def test_python_mirror(lib, vocab_bytes, dec):
    SD.check_python_mirror(lib, vocab_bytes("gpt2"), dec("dense")[1])
