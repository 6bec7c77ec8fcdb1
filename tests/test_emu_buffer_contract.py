"""`not gpu`: the device entries on the caller's buffers -- guards around every buffer, every address phase, capacities at, under and inside the result
(tests/buffer_contract_cases.py) -- on the CPU emulator (tests/hostemu/): the real kernel sources, every comparison exact against the oracle.  The emulator runs
wavefronts one after another, so a quad of d_out_ids that two wavefronts share is written in turn here: tests/test_gpu_buffer_contract.py runs the full matrix on
the hardware.  This run takes every entry, every text and every capacity kind once, the output phases in turn (buffer_contract_cases.rows(full=False))."""
import os

import pytest

import buffer_contract_cases as BC
import emu
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    return emu.library()


@pytest.fixture(scope="module")
def env(lib, oracle_mod):
    return BC.Env(lib, oracle_mod)


def test_case_layout(env):
    """The matrix is what the cases module says: every entry with every capacity kind and all four output phases, every poison and input phase on the plain
    entry and a decoder, every text with the store paths it is there for."""
    header = open(os.path.join(ROOT, "tokenizer_amd", "csrc", "tkz_kernels.h")).read()
    BC.check_layout(header, full=False)
    BC.check_layout(header, full=True)
    BC.check_inside_kinds(env)


def test_arena_reports_what_is_written():
    """the helper itself: phases from the real address, guards of 4 KiB, a store at or behind the capacity and one in front are seen"""
    mem = BC.Memory()
    for phase in BC.IDS_OUT_PHASES:
        a = BC.Arena(mem, "int32", 10, phase, 16, BC.ID_SENTINEL)
        assert a.ptr % 16 == phase and a.off >= BC.GUARD and len(a.image) - a.off - 40 >= BC.GUARD
        view = a.owner[a.off:a.off + 48].view("int32")
        assert (a.owner.view("uint8") == a.image).all() and (view == -7).all()
        view[:4] = [1, 2, 3, 4]
        assert a.read().guards_ok and a.payload[:4].tolist() == [1, 2, 3, 4] and a.tail_ok(4) and not a.tail_ok(3)
        view[10] = 5                                                    # at the capacity
        assert not a.read().behind_ok and a.front_ok and a.where() == 40
        view[10] = -7
        a.owner[a.off - 1] = 0                                          # the last byte in front
        assert not a.read().front_ok and a.behind_ok and a.where() == -1
    b = BC.Arena(mem, "uint8", 5, 48, 64, BC.np.uint8(0xE4), data=BC.np.frombuffer(b"hello", "uint8"))
    assert b.ptr % 64 == 48 and bytes(b.owner[b.off - 3:b.off + 8]) == b"\xe4\xe4\xe4hello\xe4\xe4\xe4" and b.read().unchanged()
    c = BC.Arena(mem, "int64", 0, 8, 16, BC.I64_SENTINEL)
    assert c.ptr % 16 == 8 and c.read().guards_ok and c.tail_ok(0) and len(c.payload) == 0


@pytest.mark.parametrize("entry", BC.ENTRIES)
def test_output_phase_and_capacity(env, entry):
    kinds = set()
    for name in BC.TEXT_NAMES:
        kinds |= BC.run_rows(env, entry, name, BC.rows(entry, name, full=False))
    assert kinds == set(("exact",) if entry in BC.NO_CAPACITY else BC.CAP_KINDS)


@pytest.mark.parametrize("entry", BC.INPUT_MATRIX_ENTRIES)
def test_poison_and_input_phase(env, entry):
    for name in BC.TEXT_NAMES:
        BC.run_rows(env, entry, name, BC.input_rows(entry, name, full=False))


@pytest.mark.parametrize("pattern", BC.END_PATTERNS)
def test_where_the_text_ends(lib, oracle_mod, vocab_bytes, pattern):
    """each tail where it straddles tpos - 1 | tpos and tpos + 15 | tpos + 16 and where it ends the text there; the three poisons in turn"""
    end = BC.EndEnv(lib, oracle_mod, vocab_bytes("gpt2"), pattern, every_poison=False)
    for block in (0, 1):
        for tail in BC.TAILS:
            for doc in BC.end_docs(block, tail, full=False):
                end.check(doc)
