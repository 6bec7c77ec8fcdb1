"""`-m gpu`: cache adaptation on the pipelined host path through libtkz.so -- the scenarios of tests/adapt_host_cases.py (those of tests/test_emu_adapt_host.py),
each in a child interpreter of its own, under its own time limit, with 64 KiB chunks.  The cut is made visible by $TKZ_TRACE_HOST's line; the page-locked scenario
prints Encoder.engine_downloads beside it."""
import pytest

import adapt_host_cases as AH

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scenario", AH.SCENARIOS)
def test_adapt_host(oracle_mod, scenario):
    AH.child(scenario, "gpu", timeout=120)
