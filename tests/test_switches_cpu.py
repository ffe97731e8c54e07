"""The environment switches are declared once per side and read in one place per side; README.md lists exactly the declared ones.

Source scans over the repository's own text: the C table is csrc/host_support.h (read through mnn_switch_set / mnn_switch_int, defined in
elementwise.hip), the Python table is multinn_amd/switches.py (flag / value)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multinn_amd")
CSRC = os.path.join(PKG, "csrc")

ACCESSOR_FILE = "elementwise.hip"                                  # defines mnn_switch_set / mnn_switch_int
ENVIRON_FILES = {"switches.py", "_lib.py", "build.py"}              # _lib.py: MULTINN_HIP_LIB, build.py: HIPCC -- paths, not switches
# MNN_* / MULTINN_* tokens the switch section of README.md may hold that are no switches (ABI macros, flag bits): none at present
NOT_SWITCHES = set()


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _c_switches():
    text = _read(os.path.join(CSRC, "host_support.h"))
    table = text[text.index("#define MNN_SWITCHES(X)"):text.index("enum MnnSwitch")]
    names = re.findall(r"^\s*X\((\w+),\s*\"[^\"]+\"\)", table, re.M)
    assert len(names) >= 15 and len(names) == len(set(names)), names
    return {"MNN_" + n for n in names}


def _py_switches():
    from multinn_amd import switches
    for s in switches.SWITCHES.values():
        assert s.name.startswith("MULTINN_") and s.kind in ("bool", "int", "float", "str", "path") and s.meaning, s
    return set(switches.SWITCHES)


def test_getenv_only_in_the_accessor():
    users = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if p.endswith((".hip", ".h")) and "getenv(" in _read(p)]
    assert users == [ACCESSOR_FILE], users
    # ... and a switch is read only by name of its table entry: no source spells a variable out
    spelled = {os.path.basename(p): sorted(set(re.findall(r"\"(MNN_[A-Z0-9_]+)\"", _read(p)))) for p in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))}
    assert not {f: v for f, v in spelled.items() if v}, spelled


def test_os_environ_only_in_the_switch_table():
    users = {os.path.basename(p) for p in glob.glob(os.path.join(PKG, "*.py")) if "os.environ" in _read(p)}
    assert users <= ENVIRON_FILES and "switches.py" in users, users
    # every name the package reads through flag() / value() is declared
    declared = _py_switches()
    for p in glob.glob(os.path.join(PKG, "*.py")):
        for name in re.findall(r"\b(?:flag|value)\(\"(\w+)\"\)", _read(p)):
            assert name in declared, (os.path.basename(p), name)


def test_readme_lists_exactly_the_declared_switches():
    readme = _read(os.path.join(ROOT, "README.md"))
    declared = _c_switches() | _py_switches()
    missing = sorted(n for n in declared if not re.search(r"\b%s\b" % n, readme))
    assert not missing, missing
    start = readme.index("## Environment switches")
    nxt = re.search(r"^## ", readme[start + 3:], re.M)
    section = readme[start:start + 3 + nxt.start()] if nxt else readme[start:]
    tokens = set(re.findall(r"\b(?:MNN|MULTINN)_[A-Z0-9_]+\b", section))
    assert tokens >= declared, sorted(declared - tokens)
    unknown = sorted(tokens - declared - NOT_SWITCHES)
    assert not unknown, unknown
