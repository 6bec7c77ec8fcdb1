"""`not gpu`: EncodeTrimSuffix / EncodeTrimPrefix for one string in a single launch (tkz_encode_trim_utf8 / _utf16, k_small's trim form) -- the real kernel
sources on the CPU emulator (tests/hostemu/), exact against the oracle, one text per call.  tests/test_gpu_small_trim.py runs the same cases on the hardware:
every maximum of the sweep, every seam on both of its sides, every pairing of vocabulary and pattern."""
import emu
import pytest

import small_trim_cases as ST
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


@pytest.mark.parametrize("name,pattern", [("gpt2", 1), ("synth100k", 2), ("synth200k", 3), ("synth200k", 4)])
def test_sweep_of_the_maximum(lib, vocabs, oracle_mod, name, pattern):
    ST.check_sweep(lib, oracle_mod, *vocabs(name), name, pattern, full=False)


@pytest.mark.parametrize("pattern", SC.PATTERNS)
def test_items_are_never_split(lib, vocabs, oracle_mod, pattern):
    ST.check_items(lib, oracle_mod, *vocabs("gpt2"), pattern)


@pytest.mark.parametrize("pattern", SC.PATTERNS)
def test_seams_of_the_cut(lib, vocabs, oracle_mod, pattern):
    ST.check_seams(lib, oracle_mod, *vocabs("gpt2"), pattern, full=False)


@pytest.mark.parametrize("pattern", (1, 2, 3))
def test_cut_units(lib, vocabs, oracle_mod, pattern):
    ST.check_units(lib, oracle_mod, *vocabs("gpt2"), pattern)


@pytest.mark.parametrize("pattern", (1, 3))
def test_route_limits(lib, vocabs, oracle_mod, pattern):
    ST.check_limits(lib, oracle_mod, *vocabs("gpt2"), pattern)


@pytest.mark.parametrize("pattern", (1, 2))
def test_hand_back(lib, vocabs, oracle_mod, pattern):
    ST.check_hand_back(lib, oracle_mod, *vocabs("gpt2"), pattern)


@pytest.mark.parametrize("pattern", SC.PATTERNS)
def test_utf16_entry(lib, vocabs, oracle_mod, pattern):
    ST.check_u16(lib, oracle_mod, *vocabs("gpt2"), pattern)


def test_arguments_and_capacity(lib, vocabs, oracle_mod):
    ST.check_arguments(lib, oracle_mod, *vocabs("gpt2"))


@pytest.mark.parametrize("name,pattern", [("gpt2", 1), ("synth100k", 2), ("synth200k", 3), ("synth200k", 4)])
def test_agreement_with_the_batch_entry(lib, vocabs, oracle_mod, name, pattern):
    ST.check_agreement(lib, oracle_mod, *vocabs(name), name, pattern, n_docs=4)


@pytest.mark.parametrize("pattern", [N.P1, N.CL100K])
def test_trim_and_plain_single_calls_side_by_side(lib, vocabs, oracle_mod, pattern):
    ST.check_threads(lib, oracle_mod, *vocabs("gpt2"), pattern)


def test_python_mirror(lib, vocab_bytes, oracle_mod):
    ST.check_python_mirror(lib, oracle_mod, vocab_bytes("synth100k"))
