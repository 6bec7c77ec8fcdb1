"""`not gpu`: the oracle's split (oracle/tkz_oracle.c) against V8, the regex engine the TypeScript reference compiles its patterns with
(tokenizer_ts/src/tikTokenizer.ts:100) -- the one engine of the reference that could be run while the fixtures were made.  For TKZ_PATTERN_O200K V8 is the
DEFINING engine and any well-formed text is in the domain; for pattern 1 and cl100k, which libtkz reads as .NET does, it is a reference on the texts where
the two readings coincide.  tests/golden/make_v8_fixtures.py draws the texts, applies those domain rules and records V8's pieces; no record is skipped or
filtered here.  Ids stay pinned through the oracle's BPE: the TypeScript tokenizer itself needs a newer Node than the one the fixtures were made with."""
import numpy as np
import pytest

import v8_cases as V


def starts_of(oracle_mod, pattern, b):
    return [a for a, _n in oracle_mod.split_utf8(pattern, b)]


@pytest.mark.parametrize("table", V.TABLES)
@pytest.mark.parametrize("pattern", V.PATTERNS)
def test_oracle_split_equals_v8(oracle_mod, pattern, table):
    recs = V.records(pattern, table)
    assert len(recs) >= 1000
    try:
        if table == "v8":
            oracle_mod.set_unicode_classes(V.table_for(pattern))
        for r in recs:
            assert starts_of(oracle_mod, pattern, r["bytes"]) == r["starts"], (pattern, table, r["text"][:80])
    finally:
        oracle_mod.set_unicode_classes(None)


def test_fixture_covers_the_shapes():
    """What the device tests rely on the fixture to hold: every document length around the 64-byte rows and the 4 KiB blocks, a multi-byte char across
    byte 64 and byte 4096, and for every (pattern, table) the same number of records."""
    fx = V.fixture()
    assert set(fx["header"]["pattern_sha256"]) == {"1", "2", "3"} and fx["header"] == {k: V.versions()[k] for k in fx["header"]}
    for pattern in V.PATTERNS:
        for table in V.TABLES:
            recs = V.records(pattern, table)
            docs = [r for r in recs if r["kind"] == "doc"]
            lens = {len(r["bytes"]) for r in docs}
            assert lens >= {63, 64, 65, 127, 128, 129, 1000, 4095, 4096, 4097, 9000}, (pattern, table, sorted(lens))
            assert any(len(r["bytes"]) > 64 and (r["bytes"][64] & 0xC0) == 0x80 for r in docs)
            assert any(len(r["bytes"]) > 4096 and (r["bytes"][4096] & 0xC0) == 0x80 for r in docs)
            assert all(len(r["text"]) <= 40 for r in recs if r["kind"] == "short")
            for r in recs:
                assert r["starts"] == sorted(set(r["starts"])) and (not r["bytes"] or r["starts"][0] == 0)


def test_the_two_tables_differ():
    """The census: V8's Unicode data is newer than the built-in table's, so the "v8" records can tell whether a table was honoured."""
    census = V.versions()["census"]
    changed = V.changed_code_points()
    assert census["code_points_classed_differently"] == len(changed) > 0
    assert {w["cp"] for w in census["whitespace_differences"]} >= {"U+0085", "U+FEFF"}
    tab = V.v8_table()
    assert tab[0x85] == 0 and tab[0xFEFF] == 8 and not tab[0xD800:0xE000].any() and tab.max() == 8


@pytest.mark.parametrize("pattern", V.PATTERNS)
def test_v8_records_need_the_v8_table(oracle_mod, pattern):
    """Under the BUILT-IN table the oracle cuts at least one of the "v8" records that hold a re-classed code point differently from V8 (and all of them as
    V8 does under V8's table: test_oracle_split_equals_v8) -- the "v8" mode does depend on the table."""
    recs = V.table_sensitive_records(pattern)
    assert len(recs) >= 100
    oracle_mod.set_unicode_classes(None)
    assert sum(1 for r in recs if starts_of(oracle_mod, pattern, r["bytes"]) != r["starts"]) > 0
