"""The environment variables libphifem_hip.so reads: one header holds them all, and DESIGN.md section 8 lists the same
names.  No GPU needed: the sources and the document are read as text."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phifem_amd", "csrc")
HEADER = "phx_switches.h"

KEPT = {
    "PHX_KR_IDENTITY", "PHX_KR_REDUCED", "PHX_BOX_SLOTS",
    "PHX_INNER_BOX",
    "PHX_POOL_LIMIT_GB", "PHX_DET_LIMIT_GB",
    "PHX_DIST_OVERLAP", "PHX_DIST_FUSED_PACK", "PHX_DIST_TIMEOUT_S", "PHX_RCCL_LIB",
}


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _header_names():
    text = _read(os.path.join(CSRC, HEADER))
    calls = re.findall(r"getenv\(([^)]*)\)", text)
    assert calls, "the header reads no variable"
    names = set()
    for arg in calls:
        m = re.fullmatch(r'\s*"(PHX_[A-Z0-9_]+)"\s*', arg)
        assert m, f"getenv argument is not a literal PHX_* name: {arg!r}"
        names.add(m.group(1))
    return names


def _design_table_names():
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    m = re.search(r"^## 8\..*?(?=^## )", text, re.S | re.M)
    assert m, "DESIGN.md has no section 8"
    rows = [l for l in m.group(0).splitlines() if l.startswith("|")]
    head = [i for i, l in enumerate(rows) if re.match(r"\|\s*variable\s*\|\s*default\s*\|\s*read\s*\|\s*purpose\s*\|", l)]
    assert len(head) == 1, "section 8 needs exactly one table headed variable | default | read | purpose"
    names = []
    for l in rows[head[0] + 2:]:
        cells = [c.strip() for c in l.strip().strip("|").split("|")]
        m2 = re.fullmatch(r"`(PHX_[A-Z0-9_]+)`", cells[0])
        if not m2:
            break   # the next table of the section
        assert len(cells) == 4 and all(cells), f"incomplete row: {l}"
        names.append(m2.group(1))
    assert len(names) == len(set(names)), "a switch is listed twice"
    return set(names)


def test_only_the_header_calls_getenv():
    offenders = []
    for dirpath, _, files in os.walk(CSRC):
        for name in files:
            if name == HEADER and dirpath == CSRC:
                continue
            path = os.path.join(dirpath, name)
            try:
                text = _read(path)
            except UnicodeDecodeError:
                continue   # a build product
            if "getenv(" in text:
                offenders.append(os.path.relpath(path, ROOT))
    assert not offenders, f"getenv( outside {HEADER}: {offenders}"


def test_header_matches_design_table():
    assert _header_names() == _design_table_names()


def test_kept_switches_are_exactly_the_ten():
    assert _header_names() == KEPT
