"""CPU (SIMT emulator): the exponential moving average of the weights inside cfd_fno_adam_step_ema -- tests/ema_checks.py on the unmodified
kernels, on hostile memory between guard bands.  The GPU twin is tests/test_gpu_fno_ema.py.  Every test calls the new entry point."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from tests import ema_checks as EC
from tests.backends import NumpyBackend

ROOT = Path(__file__).resolve().parent.parent
ROW = EC.register_alignment_row()  # (while pytest collects: the table of tests/align_checks.py has the new entry's row before any test runs)


@pytest.fixture(scope="module")
def be():
    return NumpyBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one -- an EMA element past n -- fails the test."""
    yield
    be.verify()


@pytest.mark.parametrize("n", EC.FLAT_NS)
def test_the_average_follows_the_rule(be, n):
    """(a) Adam and AdamW, with and without clipping, decays 0, 0.5, 0.999, three steps: within 2^-23 max(|e|, |p|) of the fp64 rule;
    decay 0 copies the parameters bit for bit."""
    assert EC.check_rule_flat(be, n) <= 1.0


@pytest.mark.parametrize("n", EC.FLAT_NS)
def test_no_other_bit_moves(be, n):
    """(b) parameters, moments, gradient and clip buffer: with an EMA == with ema = NULL == cfd_fno_adam_step."""
    EC.check_no_other_bit_moves(be, n)


def test_misplaced_buffers_give_the_aligned_bits(be):
    """(c) all buffers 4 bytes off the 16-byte grid, and the EMA alone off it."""
    EC.check_misplaced(be)


def _run_child(row_id):
    """tests/test_emul_alignment.py's run_child with this feature's child module, whose table has the row."""
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=0", PYTHONPATH=str(ROOT))
    cp = subprocess.run([sys.executable, "-m", "tests.ema_checks", "--sanitize", row_id], cwd=ROOT, env=env, capture_output=True, text=True)
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
    """(c) the same on the -fsanitize=alignment build, in a child process as tests/test_emul_alignment.py runs its rows: every placement of
    the row "adam_step_ema" -- all buffers shifted by 4 and by 8 bytes, each buffer alone by 4 -- without one report."""
    from tests import align_checks as A
    from tests.emul.build_emul import build
    from tests.test_emul_alignment import reports
    build(sanitize=True)
    row = ROW
    want = A.placements(row, True)
    assert "each4" in want
    rc, lines, err = _run_child(row.id)
    for placement in want:
        mine = err.get(placement, [])
        assert placement in lines, f"the child died (exit status {rc}) in {placement}:\n" + "\n".join(reports(mine) or mine[-15:])
        assert not reports(mine), "\n".join(reports(mine))
        assert lines[placement]["error"] is None, lines[placement]["error"]
    assert rc == 0, rc


@pytest.mark.parametrize("clip", [False, True], ids=["job_in_adam", "job_in_gradsq"])
def test_the_lifting_layers_rows(be, clip):
    """(d) 64 x 64, C = 20, L = 2, nmse, flags = 7: the fc0 ranges of the EMA obey the rule on both routes."""
    EC.check_stem_rows(be, clip)


def test_a_skipped_step_keeps_the_average(be):
    """(e)"""
    EC.check_guard(be)


def test_accumulate_ignores_the_average(be):
    """(f)"""
    EC.check_accumulate_ignores_the_ema(be)


def test_bad_decays_are_refused_before_any_launch_and_empty_buffers_write_nothing(be):
    """(f) ema_decay = 1, -0.1, NaN: CFD_ERR_INVALID_ARG, every buffer keeps its bits; n == 0: the EMA stays poison."""
    assert EC.check_bad_decay(be) == {str(d): (-1, True) for d in EC.BAD_DECAYS}
    assert EC.check_empty(be) == (True, [0.0, 1.0])
