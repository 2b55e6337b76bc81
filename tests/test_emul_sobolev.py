"""CPU (SIMT emulator): cfd_sobolev_fwd / cfd_sobolev_bwd -- tests/sobolev_checks.py on the unmodified kernels, on hostile memory between
guard bands.  The GPU twin is tests/test_gpu_sobolev.py."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from tests import sobolev_checks as SC
from tests.backends import NumpyBackend

ROOT = Path(__file__).resolve().parent.parent
ROW = SC.register_alignment_row()  # (while pytest collects: the table of tests/align_checks.py has the new entries' row before any test runs)


@pytest.fixture(scope="module")
def be():
    return NumpyBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    be.verify()


@pytest.mark.parametrize("setting", list(SC.SETTINGS))
@pytest.mark.parametrize("shape", SC.EMUL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_value_sums_and_gradient_within_the_bound(be, shape, setting):
    """(a) with and without mask and gadd, upstream by value, by device pointer and both, gpreds aliasing gadd."""
    SC.check_parity(be, shape, setting)


@pytest.mark.parametrize("setting", list(SC.SETTINGS))
def test_two_calls_on_dirty_buffers_give_the_same_bits(be, setting):
    """(b)"""
    assert SC.check_twice(be, (3, 2, 5, 7), setting) == 0
    assert SC.check_twice(be, (2, 2, 17, 36), setting) == 0


def test_misplaced_buffers_give_the_aligned_bits(be):
    """(b) every buffer 4 and 8 bytes off the 16-byte grid, and single buffers alone: the scalar loads give the 16-byte loads' bits."""
    assert SC.check_misplaced(be) == 0


def _run_child(row_id):
    """tests/test_emul_alignment.py's run_child with this feature's child module, whose table has the row."""
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=0", PYTHONPATH=str(ROOT))
    cp = subprocess.run([sys.executable, "-m", "tests.sobolev_checks", "--sanitize", row_id], cwd=ROOT, env=env, capture_output=True, text=True)
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


def test_placement_under_the_alignment_sanitizer():
    """(b) the same on the -fsanitize=alignment build, in a child process as tests/test_emul_alignment.py runs its rows: every placement of
    the row "sobolev" -- all buffers shifted by 4 and by 8 bytes, each buffer alone by 4 -- without one report."""
    from tests import align_checks as A
    from tests.emul.build_emul import build
    from tests.test_emul_alignment import reports
    build(sanitize=True)
    want = A.placements(ROW, True)
    assert "each4" in want
    rc, lines, err = _run_child(ROW.id)
    for placement in want:
        mine = err.get(placement, [])
        assert placement in lines, f"the child died (exit status {rc}) in {placement}:\n" + "\n".join(reports(mine) or mine[-15:])
        assert not reports(mine), "\n".join(reports(mine))
        assert lines[placement]["error"] is None, lines[placement]["error"]
    assert rc == 0, rc


def test_the_row_reaches_both_entry_points():
    from tests import align_checks as A
    assert {"cfd_sobolev_fwd", "cfd_sobolev_bwd"} <= A._calls_of(ROW.fn)


def test_an_exactly_predicted_sample_has_gradient_zero(be):
    """(c)"""
    SC.check_exact_sample(be)


def test_an_all_zero_label_sample(be):
    """(c) a non-finite value; the other samples' gradients stay finite and within the bound."""
    SC.check_zero_label(be)


def test_refusals_leave_every_buffer_untouched(be):
    """(c) CFD_ERR_INVALID_ARG / CFD_ERR_UNSUPPORTED before any launch."""
    res = SC.check_refusals(be)
    assert res and res == SC.expected_refusals(res), res


def test_a1_zero_is_the_rel_l2_kernels_value(be):
    """(d) Parseval across the two kernel families, on the same buffers."""
    fig, bound = SC.check_parseval(be)
    assert fig <= bound <= SC.CEILING, (fig, bound)
