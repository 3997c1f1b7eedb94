"""Where the native library's host plumbing lives, checked on the source text alone (no import of the library): the ``BBH_*``
environment is read in ONE function (``bbh_read_switches``, called by ``bbh_create`` - what ``engine._pool_key`` and INTEGRATION.md
promise: a handle reads its switches when it is created), a kernel's dynamic-LDS limit is raised in ONE helper (``bbh_allow_lds``,
per kernel and device), and the switch table of KERNELS.md section 4.5 lists exactly the switches that function reads."""

import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "baybe_amd" / "csrc"
SOURCES = sorted(list(CSRC.glob("*.hip")) + list(CSRC.glob("*.h")))

# Names in the table of KERNELS.md section 4.5 that bbh_read_switches does not read: Python-side switches (engine.py, nehvi.py,
# recommenders.py, bench.py) and compile-time macros of the kernels.
NOT_NATIVE_RUNTIME = {
    "BBH_LEAN_LBFGSB",    # engine.py: scipy.optimize.minimize instead of the engine's own loop
    "BBH_COLLECTIVE",     # bench.py: the exchange through torch.distributed
    "BBH_NEHVI_STREAMS",  # nehvi.py: one stream per target
    "BBH_NEHVI_HOST",     # nehvi.py: the host set-up
    "BBH_FAST_SOBOL",     # engine.py: torch's Sobol engine itself
    "BBH_DIAG_DPP",       # compile time (bbh_tiles.h)
    "BBH_PENDING_FAST",   # compile time (bbh_acq.hip)
}


def _function_span(path: Path, signature: str):
    """(first, last) 1-based line numbers of the function whose definition line starts with ``signature`` (ends at the next line
    that is a lone closing brace)."""
    lines = path.read_text().splitlines()
    starts = [i for i, ln in enumerate(lines) if ln.startswith(signature)]
    assert len(starts) == 1, (path.name, signature, starts)
    end = next(i for i in range(starts[0], len(lines)) if lines[i] == "}")
    return starts[0] + 1, end + 1


def _occurrences(word: str):
    return [(p.name, i + 1) for p in SOURCES for i, ln in enumerate(p.read_text().splitlines()) if word in ln]


def _only_inside(word: str, signature: str):
    first, last = _function_span(CSRC / "bbh_api.hip", signature)
    hits = _occurrences(word)
    assert hits, word
    outside = [(f, n) for f, n in hits if f != "bbh_api.hip" or not first <= n <= last]
    assert not outside, f"{word} outside {signature.strip()} (bbh_api.hip:{first}-{last}): {outside}"


def test_the_environment_is_read_in_one_function():
    _only_inside("getenv", "static bbh_switches bbh_read_switches()")


def test_the_lds_limit_is_raised_in_one_helper():
    _only_inside("hipFuncSetAttribute", "hipError_t bbh_allow_lds(")


def _table_names():
    first, last = _function_span(CSRC / "bbh_api.hip", "static bbh_switches bbh_read_switches()")
    body = "\n".join((CSRC / "bbh_api.hip").read_text().splitlines()[first - 1:last])
    return set(re.findall(r'"(BBH_[A-Z0-9_]+)"', body))


def _documented_names():
    text = (ROOT / "KERNELS.md").read_text()
    section = text[text.index("### 4.5 A/B switches"):]
    nxt = re.search(r"^#{1,3} ", section[4:], flags=re.M)
    section = section[: nxt.start() + 4] if nxt else section
    rows = [ln for ln in section.splitlines() if ln.startswith("|")]
    assert len(rows) > 20
    return set(re.findall(r"`(BBH_[A-Z0-9_]+)", "\n".join(rows)))


def test_the_documented_switches_are_the_ones_the_library_reads():
    native, documented = _table_names(), _documented_names()
    assert len(native) >= 40
    assert NOT_NATIVE_RUNTIME <= documented, NOT_NATIVE_RUNTIME - documented
    assert not NOT_NATIVE_RUNTIME & native
    missing_rows = native - documented
    stale_rows = documented - NOT_NATIVE_RUNTIME - native
    assert not missing_rows, f"switches without a row in KERNELS.md section 4.5: {sorted(missing_rows)}"
    assert not stale_rows, f"rows of KERNELS.md section 4.5 that no code reads: {sorted(stale_rows)}"


def test_switches_are_written_by_the_reader_only():
    common = (CSRC / "bbh_common.h").read_text()
    struct = common[common.index("struct bbh_switches {"):]
    struct = struct[: struct.index("\n};")]
    members = re.findall(r"^\s+(?:bool|int) (\w+) = [^;]+;", struct, flags=re.M)
    assert len(members) >= 40 and len(set(members)) == len(members)
    # every member is filled by exactly the table (no member without a row, no row without a member)
    first, last = _function_span(CSRC / "bbh_api.hip", "static bbh_switches bbh_read_switches()")
    api_lines = (CSRC / "bbh_api.hip").read_text().splitlines()
    in_table = re.findall(r"&S::(\w+)", "\n".join(api_lines[first - 1:last]))
    assert sorted(in_table) == sorted(members)
    # no assignment, compound assignment, increment or decrement of a member anywhere (the reader stores through member pointers)
    name = "|".join(members)
    write = re.compile(rf"(?:\bsw\.(?:{name})\s*(?:=(?!=)|[-+*/|&^%]=|<<=|>>=|\+\+|--))|(?:(?:\+\+|--)\s*[\w>.-]*\bsw\.(?:{name})\b)")
    whole = re.compile(r"(?:->|\.)sw\s*=(?!=)")  # the struct as a whole: bbh_create's one assignment
    writes, wholes = [], []
    for p in SOURCES:
        for i, ln in enumerate(p.read_text().splitlines()):
            code = ln.split("//")[0]
            if write.search(code):
                writes.append((p.name, i + 1, ln.strip()))
            if whole.search(code):
                wholes.append((p.name, ln.strip()))
    assert not writes, writes
    assert wholes == [("bbh_api.hip", "h->sw = bbh_read_switches();")], wholes
