"""DESIGN.md's table of environment switches against the code, in both directions (reads files only)."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NAME = r"SQUID_[A-Z0-9_]+"


def _text(paths):
    return "\n".join(p.read_text(errors="replace") for p in paths if p.is_file())


def _rows():
    design = (ROOT / "DESIGN.md").read_text()
    section = design.split("### Environment switches", 1)[1].split("\n## ", 1)[0]
    return set(re.findall(r"^\| `(" + NAME + r")` \|", section, re.M))


def test_switch_table_matches_the_code():
    rows = _rows()
    csrc = _text(sorted((ROOT / "squid_amd" / "csrc").iterdir()))
    python = _text(sorted((ROOT / "squid_amd").glob("*.py")) + [ROOT / "bench.py"])
    users = _text(sorted((ROOT / "tests").glob("*.py")) + sorted((ROOT / "tools").iterdir()) + [ROOT / "__graft_entry__.py"])
    assert rows, "no table under 'Environment switches' in DESIGN.md"
    # 1. every switch the native sources name is a row
    assert set(re.findall('"(' + NAME + ')"', csrc)) - rows == set()
    # 2. every switch a test, a tool, bench.py or the Python package mentions is a row
    assert set(re.findall(NAME, users + python)) - rows == set()
    # 3. every row is read somewhere: the native sources (build/squid's own reads included), the Python package or bench.py
    read = set(re.findall('"(' + NAME + ')"', csrc)) | set(re.findall(r"""environ[^\n]*?["'](""" + NAME + r""")["']""", python))
    assert rows - read == set()
