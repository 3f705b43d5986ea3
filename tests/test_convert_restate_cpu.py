"""CPU suite: the restatement of `genomic_regions bed` and `reg` (tests/convert_restate.py) against the hand-derived manifest
(tests/golden/convert_manifest.json), what the manifest must cover, and the restatement's notion of a plain line on the seeded
files the other conversion tests use."""
import json
import os

import pytest

import convert_restate as cr
from convert_cases import OPS, seeded_lines

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "convert_manifest.json")))["cases"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_gives_the_manifest_output(case):
    assert cr.run(case["op"], "".join(l + "\n" for l in case["input"]), case["fmt"]) == (case["stdout"], case["stderr"], case["code"])
    assert "derived by hand" in case["source"]


def test_manifest_covers_what_it_must():
    assert len(CASES) >= 30 and len({c["name"] for c in CASES}) == len(CASES)
    sam = [l.split("\t") for c in CASES if c["fmt"] == "sam" for l in c["input"] if not l.startswith("@")]
    assert {"0", "16", "83", "99", "147", "163", "2064"} <= {t[1] for t in sam}
    assert {"0", "1"} <= {t[3] for t in sam}
    assert {"*", "5S40M5S", "10M2I10M", "10M3D10M", "5H20M", "10M100N10M"} <= {t[5] for t in sam}
    spliced = [c["op"] for c in CASES if any("10M100N10M" in l for l in c["input"])]
    assert {"to": "bed"} in spliced and {"to": "reg"} in spliced and {"to": "reg", "compact": True} in spliced
    gff = [l.split("\t") for c in CASES if c["fmt"] == "gff" for l in c["input"] if not l.startswith("##")]
    assert {8, 9, 10} <= {len(t) for t in gff} and any(len(t) >= 9 and " " in t[8] for t in gff)
    bed = {len(l.split("\t")) for c in CASES if c["fmt"] == "bed" and c["op"]["to"] == "reg" for l in c["input"]}
    assert {3, 4, 5, 6} <= bed
    chr_names = {l.split("\t")[2] for c in CASES if c["op"].get("chr") for l in c["input"]}
    assert {"MT", "1", "chrX"} <= chr_names
    assert any(c["op"].get("color") == "255,0,0" for c in CASES)
    titled = [c for c in CASES if c["op"].get("title") and c["op"].get("position")]
    assert any(c["stdout"] == "" for c in titled) and any(c["stdout"].startswith("browser position ") for c in titled)
    hidden = {c["fmt"] for c in CASES if c["input"][0][:1] in "@#" or c["input"][0].startswith(("track ", "browser "))}
    assert hidden == {"sam", "gff", "bed"}


@pytest.mark.parametrize("fmt", cr.FORMATS)
def test_seeded_files_mix_plain_and_other_lines_and_hold_no_error(fmt):
    text = seeded_lines(fmt, 5)
    lines = text.split("\n")[:-1]
    assert len(lines) == 3000 and cr.is_plain(lines[0], fmt)
    assert sum(not cr.is_plain(l, fmt) for l in lines) >= 1000
    for op in OPS[fmt]:
        out, err, code = cr.run(op, text, fmt)
        assert (err, code) == ("", 0) and out.count("\n") == 3000 + (2 if op.get("title") else 0)


def test_plain_lines_are_those_the_header_names():
    sam = "q\t0\tchr1\t5\t30\t10M\t*\t0\t0\t*\t*"
    assert cr.is_plain(sam, "sam")
    for odd in (sam.replace("10M", "5M10N5M"), sam.replace("10M", "10="), sam.rsplit("\t", 1)[0], sam + "\r", sam.replace("q\t", "q r\t"),
                sam.replace("\t5\t", "\t2147483640\t"), sam.replace("10M", "10S")):
        assert not cr.is_plain(odd, "sam"), odd
    assert cr.is_plain(sam.replace("\t5\t", "\t2147483636\t"), "sam")       # STOP = 2^31 - 3, the largest the tokenizer takes
    gff = "chr1\ts\tf\t4\t9\t.\t+\t.\tl"
    assert cr.is_plain(gff, "gff") and cr.is_plain(gff[:-2], "gff") and cr.is_plain(gff + "\tc", "gff")
    for odd in (gff.replace("\t+\t", "\t.\t"), gff + "\tc\td", gff + "\r", gff.replace("\t4\t", "\t+4\t"), gff[:-1] + " l"):
        assert not cr.is_plain(odd, "gff"), odd
    assert cr.is_plain("chr1\t1\t2\tl\t0\t-", "bed") and not cr.is_plain("chr1 1 2", "bed") and not cr.is_plain("chr1\t1\t2\tl\t0\t.", "bed")
