"""`-m gpu`: the device entries on the caller's buffers through libtkz.so -- guards of 4 KiB around every buffer, every address phase of every pointer, capacities at,
under and inside the result, eight poison bytes around the input (tests/buffer_contract_cases.py): the full matrix, and the full sweep of text ends around the
trailing row of k_pretok_rows' blocks.  Every buffer lies inside one torch.uint8 tensor of the test's own; every comparison is exact against the oracle."""
import pytest

import buffer_contract_cases as BC
from tokenizer_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return N.default_library()


@pytest.fixture(scope="module")
def upload():
    import torch
    dev = torch.device("cuda", 0)

    def up(a):
        tns = torch.from_numpy(a).to(dev)
        return tns, tns.data_ptr()
    return up


@pytest.fixture(scope="module")
def env(lib, oracle_mod, upload):
    return BC.Env(lib, oracle_mod, upload)


def test_texts_reach_their_store_paths(env):
    BC.check_inside_kinds(env)


def test_arena_on_the_device(upload):
    """the helper on a device tensor: the phase of the real address, the guards, a store behind the capacity"""
    mem = BC.Memory(upload)
    for phase in BC.IDS_OUT_PHASES:
        a = BC.Arena(mem, "int32", 10, phase, 16, BC.ID_SENTINEL)
        assert a.ptr % 16 == phase and a.ptr == a.owner.data_ptr() + a.off and a.off >= BC.GUARD
        assert a.read().guards_ok and a.tail_ok(0) and (a.payload == -7).all()
        a.owner[a.off + 40] = 1                                         # at the capacity
        assert not a.read().behind_ok and a.front_ok and a.where() == 40


@pytest.mark.parametrize("text", BC.TEXT_NAMES)
@pytest.mark.parametrize("entry", BC.ENTRIES)
def test_output_phase_and_capacity(env, entry, text):
    BC.run_rows(env, entry, text, BC.rows(entry, text))


@pytest.mark.parametrize("text", BC.TEXT_NAMES)
@pytest.mark.parametrize("entry", BC.INPUT_MATRIX_ENTRIES)
def test_poison_and_input_phase(env, entry, text):
    BC.run_rows(env, entry, text, BC.input_rows(entry, text))


@pytest.fixture(scope="module")
def end_envs(lib, oracle_mod, vocab_bytes, upload):
    cache = {}

    def get(pattern):
        if pattern not in cache:
            cache[pattern] = BC.EndEnv(lib, oracle_mod, vocab_bytes("gpt2"), pattern, upload)
        return cache[pattern]
    return get


@pytest.mark.parametrize("tail", range(len(BC.TAILS)))
@pytest.mark.parametrize("block", (0, 1))
@pytest.mark.parametrize("pattern", BC.END_PATTERNS)
def test_where_the_text_ends(end_envs, pattern, block, tail):
    end = end_envs(pattern)
    for doc in BC.end_docs(block, BC.TAILS[tail]):
        end.check(doc)
