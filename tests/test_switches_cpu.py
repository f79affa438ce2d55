"""The VR_* environment switches and their documentation name the same set: every switch the engine reads has a row in
INTEGRATION.md's environment table, and every VR_* name that opens a row there is still read by the code."""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "voitta_rag_amd" / "csrc"
DOC = (ROOT / "INTEGRATION.md").read_text(encoding="utf-8")


def _read_by_the_engine():
    names = set()
    for f in sorted(CSRC.iterdir()):
        if f.suffix in (".hip", ".cpp", ".h", ".inc"):
            names |= set(re.findall(r'getenv\("(VR_[A-Z0-9_]+)"\)', f.read_text(encoding="utf-8")))
    return names


def _first_cells():
    """The VR_* names in the first cell of each row of the environment table."""
    names = set()
    for line in DOC.splitlines():
        if line.startswith("|") and line.count("|") >= 3:
            names |= set(re.findall(r"`(VR_[A-Z0-9_]+)`", line.split("|")[1]))
    return names


def test_every_switch_the_engine_reads_is_documented():
    read = _read_by_the_engine()
    assert len(read) >= 15, read  # (the search itself works: the engine reads more than a dozen)
    missing = sorted(n for n in read if not re.search(r"\b" + n + r"\b", DOC))
    assert not missing, f"read under csrc/ but not in INTEGRATION.md: {missing}"


def test_every_documented_switch_is_still_read():
    rows = _first_cells()
    assert len(rows) >= 15, rows
    sources = [f for f in (ROOT / "voitta_rag_amd").rglob("*") if f.suffix in (".hip", ".cpp", ".h", ".inc", ".py")]
    sources.append(ROOT / "bench.py")
    text = "\n".join(f.read_text(encoding="utf-8") for f in sources)
    stale = sorted(n for n in rows if not re.search(r"\b" + n + r"\b", text))
    assert not stale, f"rows of INTEGRATION.md that no code reads: {stale}"
