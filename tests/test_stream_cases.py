"""The table of tests/stream_cases.py is complete (no GPU): every prototype of include/fotg.h that takes a `void *stream` or a
`void *after_stream` has a row or an exemption with its reason, neither names anything else, every row's entry point is defined in
the file the row names, and every row builds two different input sets of the same shapes and types."""
import os
import re

import numpy as np
import pytest

import stream_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flowonthego_amd", "csrc")


def prototypes():
    """name -> parameter list of every function prototype of include/fotg.h (comments removed)"""
    text = open(os.path.join(ROOT, "include", "fotg.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(fotg_\w+)\s*\(([^()]*)\)\s*;", text)}


def stream_taking():
    return sorted(n for n, args in prototypes().items() if re.search(r"void\s*\*\s*(after_)?stream\b", args))


def test_every_stream_taking_prototype_has_a_row_or_an_exemption():
    protos, taking = prototypes(), stream_taking()
    print("\n%d prototypes, %d take a stream: %d with rows (%d rows), %d exempt" % (len(protos), len(taking), len(SC.TABLE), len(SC.ROWS), len(SC.EXEMPT)))
    for name in taking:
        print("  %-44s %s" % (name, "exempt: " + SC.EXEMPT[name] if name in SC.EXEMPT else ", ".join(r.name for r in SC.TABLE.get(name, []))))
    from flowonthego_amd._lib import SYMBOLS
    assert set(protos) == {s[0] for s in SYMBOLS}, set(protos) ^ {s[0] for s in SYMBOLS}       # the parser reads the whole header
    assert len(taking) >= 85, len(taking)
    missing = [n for n in taking if n not in SC.TABLE and n not in SC.EXEMPT]
    assert not missing, "no row in tests/stream_cases.py and no exemption: %s" % missing
    unknown = [n for n in list(SC.TABLE) + list(SC.EXEMPT) if n not in taking]
    assert not unknown, "not a stream-taking prototype of include/fotg.h: %s" % unknown
    assert not set(SC.TABLE) & set(SC.EXEMPT)
    assert all(isinstance(r, str) and len(r) > 20 for r in SC.EXEMPT.values())


def test_every_row_names_the_file_that_defines_its_entry_point():
    have = sorted(f for f in os.listdir(CSRC) if f.startswith("fotg_") and f.endswith(".hip"))
    text = {f: open(os.path.join(CSRC, f)).read() for f in have}
    for row in SC.ROWS:
        assert row.file in text, row
        assert re.search(r"^int %s\(" % row.entry, text[row.file], flags=re.M), (row, row.file)
    # a file without a row defines no entry point that takes a stream
    for f in have:
        if f not in SC.files():
            defined = set(re.findall(r"^int (fotg_\w+)\(", text[f], flags=re.M))
            assert not defined & (set(stream_taking()) - set(SC.EXEMPT)), f


@pytest.mark.parametrize("row", SC.ROWS, ids=[r.name for r in SC.ROWS])
def test_a_row_builds_two_different_input_sets(row):
    A, B = row.build()
    assert len(A) == len(B) >= 1
    assert any(not np.array_equal(a, b, equal_nan=a.dtype.kind == "f") for a, b in zip(A, B)), row
