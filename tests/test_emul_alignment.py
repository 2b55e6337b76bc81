"""CPU: the table of tests/align_checks.py on the emulator library built with -fsanitize=alignment (tests/emul/build_emul.py:
build(sanitize=True)) -- every check on buffers shifted by 4 and by 8 bytes, and at the default placement, must hold its oracle
tolerance without one "misaligned address" report; where include/cfdbench_amd.h says an entry point refuses a placement it must refuse
it before writing anything.  The one-buffer-at-a-time sweep runs here for the rows whose launchers have an alignment gate or an
over-aligned access (Row.emul_each); the GPU file runs it for every row.

Each row runs in a child process of its own (a misaligned vector access may kill the process: one finding must not take pytest with
it); the children of the whole table are started together by a module fixture, a few at a time, and the tests read their results."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

from tests import align_checks as A

ROOT = Path(__file__).resolve().parent.parent


def run_child(row_id, placements=None, sanitize=True):
    """(returncode, {placement: result line}, {placement: stderr of that placement}) of one row in a fresh process."""
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=0", PYTHONPATH=str(ROOT))
    spec = row_id + (":" + ",".join(placements) if placements else "")
    cmd = [sys.executable, "-m", "tests.align_checks"] + (["--sanitize"] if sanitize else []) + [spec]
    cp = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    lines = {}
    for ln in cp.stdout.splitlines():
        if ln.startswith("{"):
            d = json.loads(ln)
            lines[d["placement"]] = d
    err, cur = {}, None
    for ln in cp.stderr.splitlines():
        if ln.startswith("@@ "):
            cur = ln.split()[2]
        err.setdefault(cur, []).append(ln)
    return cp.returncode, lines, err


def reports(stderr_lines):
    """The sanitizer's `file:line:col: runtime error: ...` lines."""
    return [ln for ln in stderr_lines if "runtime error:" in ln or "Sanitizer" in ln]


@pytest.fixture(scope="module")
def table():
    from tests.emul.build_emul import build
    build(sanitize=True)  # (once, before the children: they would each build it otherwise)
    with ThreadPoolExecutor(max_workers=max(1, min(6, (os.cpu_count() or 2) - 1))) as ex:
        return dict(zip((r.id for r in A.ROWS), ex.map(lambda r: run_child(r.id), A.ROWS)))


@pytest.mark.parametrize("row,placement", [(r, p) for r in A.ROWS for p in A.placements(r, True)], ids=lambda v: getattr(v, "id", v))
def test_row_on_the_sanitized_emulator(table, row, placement):
    rc, lines, err = table[row.id]
    mine = err.get(placement, [])
    assert placement in lines, f"the child died (exit status {rc}) in {row.id} {placement}:\n" + "\n".join(reports(mine) or mine[-15:])
    assert not reports(mine), "\n".join(reports(mine))
    assert lines[placement]["error"] is None, lines[placement]["error"]
    assert rc in (0, 1), rc


def test_the_default_build_is_untouched_by_the_sanitized_one():
    from tests.emul import build_emul
    a, b = build_emul.build(), build_emul.build(sanitize=True)
    assert a.parent != b.parent and a.parent == build_emul.OUT and b.parent.parent == build_emul.OUT  # (under _build: out of git with it)


def test_every_entry_point_with_a_tensor_argument_has_a_row():
    """Every exported entry point that takes a device pointer is reached by a row of the table (so: runs misaligned on both backends).
    Left out: the functions without a tensor argument -- sizes, plans, knobs, the profiler, version and error text."""
    import ctypes
    import re

    from cfdbench_amd._capi import _SIGS, FfnStackArgs
    header = (ROOT / "include" / "cfdbench_amd.h").read_text()
    declared = set(re.findall(r"^(?:int|size_t|void|const char\*)\s+(cfd_\w+)\s*\(", header, flags=re.M))
    assert declared == set(_SIGS), declared ^ set(_SIGS)
    no_tensor = {n for n in declared if n.endswith(("_bytes", "_bytes_ex", "_slots", "_supported"))} | {
        "cfd_version", "cfd_last_error", "cfd_tune_set", "cfd_prof_begin", "cfd_prof_end", "cfd_plan_create", "cfd_plan_destroy"}
    for n in no_tensor:  # (none of them has a float* / void* data argument besides the plan)
        m = re.search(r"^[a-z_ \*]+\b" + n + r"\s*\(([^;]*)\);", header, flags=re.M)
        assert m and not re.search(r"float\s*\*|void\s*\*\s*ws", m.group(1)), n
    assert ctypes.POINTER(FfnStackArgs) in _SIGS["cfd_ffn_stacks_fwd"][1]
    rows = A.entry_rows()
    unmapped = sorted(declared - no_tensor - set(rows))
    assert not unmapped, f"entry points that no row of tests/align_checks.py runs misaligned: {unmapped}"
    assert not (set(rows) - declared), set(rows) - declared


def test_every_check_function_is_a_row():
    import inspect

    from tests import chan_checks, kernel_checks, modes_checks, wide_checks
    used = {r.fn for r in A.ROWS}
    for mod in (kernel_checks, wide_checks, modes_checks, chan_checks):
        for name, fn in inspect.getmembers(mod, inspect.isfunction):
            if name.startswith("check_") and fn.__module__ == mod.__name__ and name not in A.NOT_ROWS:
                assert fn in used, f"{mod.__name__}.{name} has no row in tests/align_checks.py"


def test_every_refusal_of_the_table_is_in_the_header():
    """A row that expects a refusal names an entry point whose declaration (or the Alignment paragraph) states the alignment."""
    header = (ROOT / "include" / "cfdbench_amd.h").read_text()
    para = header[header.index("- Alignment."):header.index("- functions are re-entrant")]
    for word in ("cfd_convt2_*", "cfd_convt2_bwd_ex", "cfd_dropout_gelu_*", "statistics records", "weight fragments", "CFD_ERR_UNSUPPORTED"):
        assert word in para, word
    assert {r.id for r in A.ROWS if r.refuse} == {"conv_bn_stats", "conv_prepared", "convt", "convt_valu", "pool_convt_resid", "convt_strided",
                                                  "dropout_gelu", "dropout_step"}
    assert A.UNSUPPORTED == int(__import__("re").search(r"#define CFD_ERR_UNSUPPORTED \((-\d+)\)", header).group(1))
