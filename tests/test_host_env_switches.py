"""The environment switches: the library reads exactly the variables INTEGRATION.md's table
lists, and the switches of retired launch paths are named nowhere in the package or the tests
(no GPU, no build: the sources and the document are read as text)."""
import os
import re

from helpers import ROOT

CSRC = os.path.join(ROOT, "hmsc_amd", "csrc")
PYTHON_ONLY = {"HMSC_AMD_LIB", "HMSC_AMD_ALLOW_STALE", "HMSC_OFFLOAD_ARCH"}  # read by the binding / the build
REMOVED = [
    "HMSC_XZ_FOLD", "HMSC_G2S_SLAB", "HMSC_TAIL_DEFER_LEVELS", "HMSC_NO_PSI_PRE", "HMSC_Z_PACK_FIRST",
    "HMSC_Z_PACK_ROW", "HMSC_RED_PRIO", "HMSC_LONG_TAIL", "HMSC_FIRST_REPLAY", "HMSC_KERNEL_COPY_MAX",
    "HMSC_SINGLE_STREAM", "HMSC_SPIN_WAIT", "HMSC_NO_G2BL_FUSION", "HMSC_NO_ETA_FUSION", "HMSC_NO_SIDE_FUSION",
    "HMSC_NO_SHARD_FUSION", "HMSC_NO_SHARD_DEV", "HMSC_NO_SIDE_ROOT", "HMSC_NO_EXT_SIDE",
]
TEXT = (".py", ".hip", ".cpp", ".h", ".c", ".md", ".txt", ".sh", ".json")


def _text_files(top):
    for d, dirs, files in os.walk(top):
        dirs[:] = [x for x in dirs if x != "__pycache__"]
        for f in files:
            if f.endswith(TEXT):
                yield os.path.join(d, f)


def _read_by_library():
    names = set()
    for path in _text_files(CSRC):
        names.update(re.findall(r'\bgetenv(?:_flag)?\(\s*"(HMSC_[A-Z0-9_]+)"', open(path).read()))
    return names


def _documented():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = text[text.index("## Environment switches"):]
    rows = [ln for ln in table.splitlines() if ln.startswith("| `HMSC_")]
    names = [re.match(r"\| `(HMSC_[A-Z0-9_]+)", ln).group(1) for ln in rows]
    assert len(names) == len(set(names)), "a variable has two rows"
    for ln in rows:  # one row per variable: no second name in the first cell
        assert len(re.findall(r"HMSC_[A-Z0-9_]+", ln.split("|")[1])) == 1, ln
    return set(names)


def test_table_lists_exactly_what_the_library_reads():
    read, doc = _read_by_library(), _documented()
    assert len(read) >= 15  # (the pattern still finds the reads)
    assert PYTHON_ONLY <= doc
    assert read == doc - PYTHON_ONLY, (sorted(read - doc), sorted(doc - PYTHON_ONLY - read))


def test_retired_switches_are_named_nowhere():
    me = os.path.abspath(__file__)
    hits = []
    for top in ("hmsc_amd", "tests"):
        for path in _text_files(os.path.join(ROOT, top)):
            if os.path.abspath(path) == me:
                continue
            text = open(path, errors="replace").read()
            hits += [(os.path.relpath(path, ROOT), n) for n in REMOVED if re.search(n + r"(?![A-Z0-9_])", text)]
    assert not hits, hits
