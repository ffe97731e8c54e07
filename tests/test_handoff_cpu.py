"""The hand-off protocol of the persistent LSTM recurrences is defined once, in csrc/lstm_handoff.h.

Source scans over the repository's own text: the agent-scope access of a sync word, the XCC-id read of the XCD probe and the LDS-only
workgroup barrier are what every copy of the protocol needs, so each may occur in the header and in no other file of csrc."""
import glob
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multinn_amd", "csrc")
HEADER = "lstm_handoff.h"

MARKS = {
    "agent-scope load / store": "__HIP_MEMORY_SCOPE_AGENT",
    "XCC-id read": "HW_REG_XCC_ID",
    "LDS-only barrier": "lgkmcnt(0)\\n\\ts_barrier",          # as written in the source: the two instructions of one asm statement
}


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


@pytest.mark.parametrize("what", sorted(MARKS))
def test_defined_only_in_the_handoff_header(what):
    files = sorted(p for p in glob.glob(os.path.join(CSRC, "*")) if p.endswith((".hip", ".h")))      # the sources; a build leaves objects beside them
    assert len(files) >= 20 and os.path.join(CSRC, HEADER) in files, files
    users = [os.path.basename(p) for p in files if MARKS[what] in _read(p)]
    assert users == [HEADER], (what, users)
