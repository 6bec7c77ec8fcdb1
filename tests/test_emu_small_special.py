"""`not gpu`: Encode(text, allowedSpecial) for one string in a single launch (tkz_encode_special_utf8 / _utf16, k_small's special form) -- the real kernel
sources on the CPU emulator (tests/hostemu/), bit-exact against the oracle, one text per call.  tests/test_gpu_small_special.py runs the same cases on the
hardware, the seams at every offset."""
import emu
import pytest

import small_special_cases as SS
import special_cases as SC
from tokenizer_amd import _native as N


@pytest.fixture(scope="module")
def lib():
    return emu.library()


@pytest.fixture(scope="module")
def vocabs(lib, vocab_bytes, oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            raw = vocab_bytes(name)
            cache[name] = (N.Vocab(raw, lib), oracle_mod.Vocab(raw))
        return cache[name]
    return get


@pytest.mark.parametrize("pattern", SC.PATTERNS)
@pytest.mark.parametrize("name", list(SC.SPECIAL_SETS))
def test_edge_documents(lib, vocabs, oracle_mod, name, pattern):
    SS.check_edge_docs(lib, oracle_mod, *vocabs(name), name, pattern)


@pytest.mark.parametrize("pattern", SC.PATTERNS)
def test_registration_order_and_overlaps(lib, vocabs, oracle_mod, pattern):
    SS.check_order(lib, oracle_mod, *vocabs("gpt2"), pattern)


@pytest.mark.parametrize("pattern", SC.PATTERNS)
def test_literals_across_seams(lib, vocabs, oracle_mod, pattern):
    SS.check_seams(lib, oracle_mod, *vocabs("gpt2"), pattern, full=False)


@pytest.mark.parametrize("pattern", (1, 2, 3))
def test_literal_across_byte_65536(lib, vocabs, oracle_mod, pattern):
    SS.check_64k(lib, oracle_mod, *vocabs("gpt2"), pattern)


@pytest.mark.parametrize("pattern", SC.PATTERNS)
def test_segments(lib, vocabs, oracle_mod, pattern):
    SS.check_segments(lib, oracle_mod, *vocabs("gpt2"), pattern)


def test_literal_bytes_outside_the_vocabulary(lib, oracle_mod):
    SS.check_outside_vocabulary(lib, oracle_mod)


@pytest.mark.parametrize("pattern", (1, 2))
def test_hand_back(lib, vocabs, oracle_mod, pattern):
    SS.check_hand_back(lib, oracle_mod, *vocabs("gpt2"), pattern)


@pytest.mark.parametrize("pattern", SC.PATTERNS)
def test_utf16_entry(lib, vocabs, oracle_mod, pattern):
    SS.check_u16(lib, oracle_mod, *vocabs("gpt2"), pattern)


def test_memo_and_promotions_never_hold_a_literal(lib, vocabs, oracle_mod):
    SS.check_memo(lib, oracle_mod, *vocabs("gpt2"))


def test_limits_and_arguments(lib, vocabs, oracle_mod):
    SS.check_arguments(lib, oracle_mod, *vocabs("gpt2"))


@pytest.mark.parametrize("pattern", [N.P1, N.CL100K])
def test_special_and_plain_single_calls_side_by_side(lib, vocabs, oracle_mod, pattern):
    SS.check_threads(lib, oracle_mod, *vocabs("gpt2"), pattern)


def test_python_mirror(lib, vocab_bytes, oracle_mod):
    SS.check_python_mirror(lib, oracle_mod, vocab_bytes("synth100k"))


@pytest.mark.parametrize("name,pattern", [("gpt2", 1), ("synth100k", 2), ("synth200k", 3), ("synth200k", 4)])
def test_random_texts(lib, vocabs, oracle_mod, name, pattern):
    SS.check_random(lib, oracle_mod, *vocabs(name), name, pattern, seeds=3)
