"""Cache adaptation on the pipelined host path, on the CPU-emulated build: the scenarios of tests/adapt_host_cases.py, each in a child interpreter with
64 KiB chunks (the chunk size is read once per process).  The cut is made visible by $TKZ_TRACE_HOST's line, which every call of a scenario must have written."""
import pytest

import adapt_host_cases as AH
import emu


@pytest.fixture(scope="module")
def built():
    emu.library()              # (built once, here: the children find it ready)


@pytest.mark.parametrize("scenario", AH.SCENARIOS)
def test_adapt_host(built, oracle_mod, scenario):
    AH.child(scenario, "emu", timeout=600)
