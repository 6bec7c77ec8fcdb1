"""`not gpu`: the argument checks of the twelve host entries, row by row (tests/entry_arg_cases.py), through the emulated library: the status, what the call
leaves in *needed and what tkz_encoder_special_stats moved by are literals of the table.  tests/test_gpu_entry_args.py runs the same rows through libtkz.so."""
import pytest

import emu
import entry_arg_cases as EA


@pytest.fixture(scope="module")
def lib():
    return emu.library()


@pytest.fixture(scope="module")
def encoder(lib, gpt2_tiktoken_bytes):
    enc = EA.make_encoder(lib, gpt2_tiktoken_bytes)
    return enc, EA.base_ids(enc)


def test_the_table_covers_every_entry():
    assert {r.entry for r in EA.TABLE} == set(EA.ENTRIES) and len(EA.ENTRIES) == 12
    assert len({r.id for r in EA.TABLE}) == len(EA.TABLE)
    for entry, (kind, special, trim) in EA.ENTRIES.items():
        cases = {r.case for r in EA.TABLE if r.entry == entry}
        assert {"ok", "null_data", "negative_total", "empty_1"} <= cases, entry
        if entry not in ("tkz_pretokenize_utf8", "tkz_encode_utf16"):
            assert {"n_docs_negative", "null_offsets", "offs0_is_1", "offsets_decrease", "null_out_offsets", "null_ids", "cap_one_short", "empty_0", "empty_3"} <= cases, entry
        assert ({"allowed_out_of_range", "allowed_repeated"} <= cases) == special, entry
        assert ({"bad_side", "negative_max", "negative_per_doc"} <= cases) == trim, entry


@pytest.mark.parametrize("row", EA.TABLE, ids=lambda r: r.id)
def test_row(lib, encoder, row):
    enc, ids = encoder
    EA.check(lib, enc, ids, row)
