"""The integer records of the sweeps (box, status and sweep record) and the list capacities have ONE layout: the ASDF_BOX_* /
ASDF_STATUS_* / ASDF_REC_* / ASDF_*_CAP constants of include/alignsdf_hip.h.  The header is read as text here: every constant
must have the same value in the Python mirror (alignsdf_amd/_native.py), and the values must be the ones spelt out below - the
numbers the C ABI has had since these words were introduced.  An edit that renumbers a word fails here, without a GPU."""
import os
import re

from alignsdf_amd import _native, hip_decoder

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "alignsdf_hip.h")

EXPECTED = {
    # box record: int32[16], 8 words per head; flags in bits 29 / 30 of word 7
    "BOX_MIN": 0, "BOX_MAX": 3, "BOX_COUNT": 6, "BOX_RANGE": 7, "BOX_STRIDE": 8, "BOX_WORDS": 16,
    "BOX_CLUSTER_FAULT_BIT": 1 << 29, "BOX_NEAR_OVERFLOW_BIT": 1 << 30, "BOX_RANGE_MASK": (1 << 29) - 1,
    # status record: int32[16]
    "STATUS_RANGE": 0, "STATUS_LIST_OVERFLOW": 1, "STATUS_FIXUP": 2, "STATUS_MAX_ERR": 3, "STATUS_PEAK": 4, "STATUS_PEAK_STRIDE": 4,
    "STATUS_CLUSTER_FAULT": 11, "STATUS_CLOCK": 12, "STATUS_WORDS": 16,
    # sweep record: int32[48] = box record, status copy at 16, words 32..41
    "REC_STATUS": 16, "REC_CANDIDATES": 32, "REC_BAND": 33, "REC_AUDIT_MAX_ERR": 35, "REC_AUDIT_FLIPS": 36, "REC_AUDIT_EVALS": 37,
    "REC_NEAR_OVERFLOW": 38, "REC_SHELL_PICKS": 39, "REC_SHELL_POPULATION": 40, "REC_AUDIT_SUMSQ": 41, "REC_WORDS": 48,
    # list capacities
    "NEAR_CAP": 1 << 16, "CAND_CAP": 1 << 21, "BAND_CAP": 1 << 22,
}


def header_constants():
    with open(HEADER) as f:
        text = f.read()
    out = {}
    for name, value in re.findall(r"^#define ASDF_((?:BOX|STATUS|REC)_\w+|(?:NEAR|CAND|BAND)_CAP)\s+(\(?[0-9a-fx<\s]+\)?)\s*(?:/\*|$)", text, flags=re.M):
        m = re.fullmatch(r"\(?\s*(0x[0-9a-f]+|\d+)\s*(?:<<\s*(\d+))?\s*\)?", value.strip())
        assert m, (name, value)
        out[name] = int(m.group(1), 0) << int(m.group(2) or 0)
    return out


def test_header_layout_is_the_pinned_one():
    assert header_constants() == EXPECTED


def test_python_mirror_matches_the_header():
    for name, value in header_constants().items():
        assert getattr(_native, name) == value, name
    # the names other modules and the tests import
    assert (hip_decoder.NEAR_OVERFLOW_BIT, hip_decoder.CLUSTER_FAULT_BIT) == (0x40000000, 0x20000000)
    assert (hip_decoder.REC_WORDS, hip_decoder.NEAR_CAP, hip_decoder.CAND_CAP, hip_decoder.BAND_CAP) == (48, 1 << 16, 1 << 21, 1 << 22)
    assert _native.BOX_RANGE_WORDS == (7, 15)


def test_records_nest_as_documented():
    c = header_constants()
    assert c["BOX_WORDS"] == 2 * c["BOX_STRIDE"] and c["REC_STATUS"] == c["BOX_WORDS"] and c["REC_CANDIDATES"] == c["REC_STATUS"] + c["STATUS_WORDS"]
    assert c["BOX_RANGE_MASK"] == c["BOX_CLUSTER_FAULT_BIT"] - 1 and c["BOX_NEAR_OVERFLOW_BIT"] == 2 * c["BOX_CLUSTER_FAULT_BIT"]
    assert c["STATUS_PEAK"] + c["STATUS_PEAK_STRIDE"] + 2 < c["STATUS_CLUSTER_FAULT"] < c["STATUS_CLOCK"] and c["STATUS_CLOCK"] + 4 == c["STATUS_WORDS"]
