"""host/tokenizer.c + host/connectEngine.c:convert_conditions against what the
reference's tokenizer/parser produced for the same SQL text
(tests/golden/parse_golden.json, from oracle/_ref).  CPU only."""
import json

import pytest

import qpelib as q

CASES = json.loads((q.GOLDEN / "parse_golden.json").read_text())


@pytest.mark.parametrize("case", CASES, ids=[str(i) for i in range(len(CASES))])
def test_front_end_matches_reference(case):
    lib = q.pq.lib()
    sql = case["sql"].encode("latin-1")
    assert q.call_text(lib.hipDumpTokens, sql) == case["tokens"]
    assert q.call_text(lib.hipDumpParse, sql) == case["parse"]


def test_wide_sql_matches_reference():
    """SQL past the reference parser's five conditions per level, ten select items, a DELETE with a sub-chain: tokens and
    parse equal what the reference produced (tests/golden/parse_wide_golden.json)."""
    lib = q.pq.lib()
    for case in json.loads((q.GOLDEN / "parse_wide_golden.json").read_text()):
        sql = case["sql"].encode("latin-1")
        assert q.call_text(lib.hipDumpTokens, sql) == case["tokens"], case["sql"]
        assert q.call_text(lib.hipDumpParse, sql) == case["parse"], case["sql"]
