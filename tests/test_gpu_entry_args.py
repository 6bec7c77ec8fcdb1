"""`-m gpu`: the rows of tests/entry_arg_cases.py through libtkz.so -- the same literals as tests/test_emu_entry_args.py.  Every row is a batch of a few dozen
bytes; every bad argument is refused on the host before any launch, or reported by the device through its error bits."""
import pytest

import entry_arg_cases as EA
from tokenizer_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return N.default_library()


@pytest.fixture(scope="module")
def encoder(lib, gpt2_tiktoken_bytes):
    enc = EA.make_encoder(lib, gpt2_tiktoken_bytes)
    return enc, EA.base_ids(enc)


@pytest.mark.parametrize("row", EA.TABLE, ids=lambda r: r.id)
def test_row(lib, encoder, row):
    enc, ids = encoder
    EA.check(lib, enc, ids, row)
