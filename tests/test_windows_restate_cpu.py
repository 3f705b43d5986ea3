"""CPU suite: the restatement of `genomic_regions win` (tests/windows_restate.py) against the hand-derived manifest
(tests/golden/windows_manifest.json), and the closed forms the device path plans with -- windows per line, full-size windows,
digit sums of an arithmetic progression, bytes of a line's first k windows -- against the restated loop."""
import json
import os

import pytest

import windows_restate as wr

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "windows_manifest.json")))["cases"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_gives_the_manifest_output(case):
    assert wr.run(case["op"], "".join(l + "\n" for l in case["input"])) == (case["stdout"], case["stderr"], case["code"])


def test_manifest_covers_what_it_must():
    names = {c["name"] for c in CASES}
    cols = {len(c["input"][-1].split("\t")) for c in CASES}
    assert {3, 4, 5, 6, 7, 12} <= cols
    assert any(c["op"]["small"] for c in CASES) and any(not c["op"]["small"] for c in CASES)
    assert {c["op"]["size"] for c in CASES} >= {0, -3}
    assert {"start_behind_stop", "header_and_the_defaults", "space_separated", "twelve_columns_two_blocks_is_an_error"} <= names


STEPS = (1, 7, 10, 999, 10 ** 6)


@pytest.mark.parametrize("step", STEPS)
def test_progression_digits_around_every_power_of_ten(step):
    """every a within +-3 of each power of ten up to 10^9, m up to a few thousand, against the digits counted term by term"""
    for j in range(0, 10):
        for a in range(max(10 ** j - 3, 0), 10 ** j + 4):
            top = min(3000, (10 ** 10 - 1 - a) // step + 1)           # terms below 10^10
            want = 0
            marks = {0, 1, 2, 3, 9, 10, 11, 99, 100, 101, 142, 143, 144, 999, 1000, 1001, 1428, 1429, 2999, 3000, top}
            for m in range(0, top + 1):
                if m in marks:
                    assert wr.progression_digits(a, step, m) == want, (a, step, m)
                want += wr.digits(a + m * step)


def line_of(a, length, cols):
    return "\t".join(["chr7", str(a), str(a + length), "name", "12", "-"][:cols])


@pytest.mark.parametrize("small", [False, True], ids=["full", "small"])
@pytest.mark.parametrize("step", STEPS)
def test_counts_and_bytes_against_the_loop(step, small):
    """n, c and the bytes of the first k windows for every k, on lines whose starts sit at the powers of ten"""
    for j in (0, 1, 3, 6, 9):
        for a in (max(10 ** j - 3, 0), 10 ** j - 1 if j else 0, 10 ** j, 10 ** j + 2):
            for size, windows in ((1, 40), (25, 7), (1000, 1500)):
                for extra in sorted({0, step // 2, step - 1}):            # below the step: no window more
                    for cols in (3, 4, 5, 6):
                        if step >= 999 and windows > 40:
                            continue
                        length = size + (windows - 1) * step + extra
                        if a + length >= 2 ** 31 - 2:
                            continue
                        line = line_of(a, length, cols)
                        assert wr.is_plain(line)
                        text = wr.windows_of(wr.read_bed(line, 1), step, size, small)
                        rows = text.split("\n")[:-1]
                        assert wr.n_full(length, step, size) == windows
                        assert wr.n_windows(length, step, size, small) == len(rows)
                        if not small:
                            assert len(rows) == windows
                        at = 0
                        for k in range(len(rows) + 1):
                            if k < 60 or k % 97 == 0 or k > len(rows) - 60:
                                assert wr.bytes_before(line, step, size, small, k) == at, (line, k)
                            if k < len(rows):
                                at += len(rows[k]) + 1
                        assert all(len(r) + 1 <= wr.fixed_part(line) + 20 for r in rows)


def test_counts_of_short_and_empty_lines():
    for length in range(-3, 12):
        for step in (1, 2, 5):
            for size in (1, 4, 9):
                for small in (False, True):
                    line = line_of(20, length, 4) if length >= 0 else "chr7\t20\t%d\tname" % (20 + length)
                    rows = wr.windows_of(wr.read_bed(line, 1), step, size, small).count("\n")
                    assert wr.n_windows(length, step, size, small) == rows, (length, step, size, small)
                    assert wr.bytes_before(line, step, size, small, rows) == len(wr.windows_of(wr.read_bed(line, 1), step, size, small))
