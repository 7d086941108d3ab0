"""INTEGRATION.md §4b is the complete list of switches that change what runs: every MTTS_* / HIPCC name the
package and build_native.py read from the environment, and every MTTS_* name csrc/ reads with getenv or tests
as a build option, has a row there -- and every row names a switch the code still reads.  Text only: no GPU,
no library."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "matcha-tts-etu-upmc-ensam_amd"
NAME = r"(MTTS_[A-Z0-9_]+|HIPCC)"
# os.environ.get("X" / os.environ["X" / os.environ.setdefault("X" / os.environ.pop("X" / os.getenv("X" / "X" in os.environ
PY_READS = (re.compile(r"os\.(?:environ(?:\.\w+)?\s*[\[(]|getenv\s*\()\s*[\"']" + NAME + r"[\"']"),
            re.compile(r"[\"']" + NAME + r"[\"']\s+(?:not\s+)?in\s+os\.environ"))
# getenv("X"), and the preprocessor tests #if / #ifdef / #ifndef / #elif (defined(X) included); enum and
# flag names of the headers appear in neither construct
C_GETENV = re.compile(r"getenv\s*\(\s*\"(MTTS_[A-Z0-9_]+)\"")
C_COND = re.compile(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", re.M)
SECTION = re.compile(r"^## 4b\..*?(?=^## )", re.M | re.S)
ROW_NAME = re.compile(r"^\|\s*`" + NAME + r"`", re.M)


def names_read_by_python():
    files = [p for p in PKG.rglob("*.py") if "build" not in p.relative_to(PKG).parts[:-1]]
    assert PKG / "build_native.py" in files and len(files) > 10
    return {n for p in files for rx in PY_READS for n in rx.findall(p.read_text())}


def names_read_by_native():
    out = set()
    for p in (PKG / "csrc").iterdir():
        text = p.read_text()
        out |= set(C_GETENV.findall(text))
        for cond in C_COND.findall(text):
            out |= set(re.findall(r"\bMTTS_[A-Z0-9_]+\b", cond))
    return out


def names_in_tables():
    section = SECTION.search((ROOT / "INTEGRATION.md").read_text())
    assert section, "INTEGRATION.md has no section 4b"
    names = ROW_NAME.findall(section.group(0))
    assert len(names) == len(set(names)), "a switch has two rows"
    return set(names)


def test_documented_switches_are_the_switches_read():
    read = names_read_by_python() | names_read_by_native()
    listed = names_in_tables()
    assert {"MTTS_MAS_TR", "MTTS_LIB", "HIPCC", "MTTS_GEMM_TIMELINE"} <= read  # the scan finds all three kinds
    assert read - listed == set(), f"read by the code, no row in INTEGRATION.md 4b: {sorted(read - listed)}"
    assert listed - read == set(), f"a row in INTEGRATION.md 4b, read by no code: {sorted(listed - read)}"
