"""CPU: the hostile allocators of tests/backends.py bite.  Three deliberately broken stand-ins for a C-ABI entry point (raw pointers and
sizes, written here, not in the product) -- one leaves an output element unwritten, one adds into its output, one writes 4 bytes past
its workspace -- pass on friendly zeroed memory and are caught on out() / scratch() / by verify(); a fourth writes 4 bytes in front of a
payload placed off the 16-byte grid (be.misaligned) and is caught there too.  Also: every workspace size function
of include/cfdbench_amd.h is named by tests/kernel_checks.py: WORKSPACE_COVERAGE."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from tests import backends as BK
from tests import kernel_checks as K

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def be():
    return BK.NumpyBackend()


def _f32(ptr, n):
    return np.ctypeslib.as_array((ctypes.c_float * n).from_address(ptr))


def _u8(ptr, n):
    return np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(ptr))


def twice_skipping_the_last(x, y, n):
    """y = 2 x, but the last element is never written (a ragged tail the kernel forgot)."""
    _f32(y, n)[:n - 1] = 2.0 * _f32(x, n)[:n - 1]


def twice_accumulating(x, y, n):
    """y += 2 x where the contract says y = 2 x."""
    _f32(y, n)[:] += 2.0 * _f32(x, n)


def twice_overrunning_scratch(x, y, ws, ws_bytes, n):
    """y = 2 x through a workspace, with one float stored just past the workspace's end."""
    _u8(ws, ws_bytes + 4)[ws_bytes:] = 0
    _f32(y, n)[:] = 2.0 * _f32(x, n)


def twice_underrunning(x, y, n):
    """y = 2 x, with one float stored just in front of y (an aligned vector store at an address rounded down)."""
    _f32(y - 4, n + 1)[:] = np.concatenate([[0.0], 2.0 * _f32(x, n)])


def _parity(be, fn, alloc, n=37):
    x = np.arange(n, dtype=np.float32)[::-1].copy()  # the last element's true result is 0: zero-filled memory hides a skipped store
    dx, y = be.dev(x), alloc((n,))
    fn(be.ptr(dx), be.ptr(y), n)
    return K.nm(be.host(y), 2.0 * x.astype(np.float64))


def test_poison_is_nan_in_every_format(be):
    for dtype in (np.float32, np.complex64):
        a = be.host(be.out((5, 3), dtype))
        assert np.isnan(a.real).all() and (dtype is np.float32 or np.isnan(a.imag).all())
        h = a.view(np.uint16)
        assert ((h & 0x7F80) == 0x7F80).all() and ((h & 0x007F) != 0).all()  # bf16: exponent all ones, mantissa non-zero
    w = be.host(be.scratch(10))
    assert w.shape == (10,) and np.isnan(w[:8].view(np.float32)).all() and (w[8:].view(np.uint16) == 0x7FC0).all()
    assert be.host(be.bytes(8)).tobytes() == w[:8].tobytes()
    assert not be.host(be.zeros((4,))).any()
    assert be.ptr(be.out((3,))) % 16 == 0 and be.ptr(be.scratch(5)) % 16 == 0  # the guard keeps a plain allocation's 16-byte alignment
    be.verify()


def test_unwritten_output_element_is_caught(be):
    assert _parity(be, twice_skipping_the_last, be.zeros) < K.TOL          # friendly memory: passes although broken
    v = _parity(be, twice_skipping_the_last, be.out)
    assert not (v < K.TOL), v                                              # the comparison every check uses fails
    be.verify()


def test_accumulating_into_an_output_is_caught(be):
    assert _parity(be, twice_accumulating, be.zeros) < K.TOL
    v = _parity(be, twice_accumulating, be.out)
    assert not (v < K.TOL), v
    be.verify()


def test_overrun_of_a_workspace_is_caught(be):
    n, nbytes = 9, 40
    dx, y, ws = be.dev(np.ones(n, np.float32)), be.out((n,)), be.scratch(nbytes)
    twice_overrunning_scratch(be.ptr(dx), be.ptr(y), be.ptr(ws), nbytes, n)  # (lands in the guard band: memory this test allocated)
    assert K.nm(be.host(y), np.full(n, 2.0)) < K.TOL                          # the results are right; only the guard shows it
    with pytest.raises(AssertionError) as e:
        be.verify()
    msg = str(e.value)
    assert "scratch" in msg and "(40,)" in msg and "uint8" in msg and "back guard" in msg and "first at byte 0 " in msg and "4 byte(s)" in msg
    assert msg.count("guard band damaged") == 1                               # the inputs' and the output's guards are intact
    be.verify()                                                               # (the buffers were forgotten: nothing left to report)


def test_write_in_front_of_an_input_is_caught(be):
    dx = be.dev(np.ones((2, 3), np.complex64))
    _u8(be.ptr(dx) - 2, 2)[:] = 7
    with pytest.raises(AssertionError, match=r"dev shape=\(2, 3\) dtype=complex64: front guard band damaged, first at byte 4094 of 4096, 2 byte"):
        be.verify()


def test_write_in_front_of_a_shifted_payload_is_caught(be):
    """The guard bands follow the payload to its place: the front band of a buffer shifted by 4 bytes is 4100 bytes long and ends at it."""
    n = 9
    with be.misaligned(4):
        dx, y = be.dev(np.ones(n, np.float32)), be.out((n,))
        assert be.allocations == 2
    assert be.ptr(y) % 16 == 4
    twice_underrunning(be.ptr(dx), be.ptr(y), n)                               # (lands in the guard band: memory this test allocated)
    assert K.nm(be.host(y), np.full(n, 2.0)) < K.TOL                           # the results are right; only the guard shows it
    with pytest.raises(AssertionError) as e:
        be.verify()
    msg = str(e.value)
    assert "out shape=(9,) dtype=float32 shift=4: front guard band damaged, first at byte 4096 of 4100, 4 byte(s)" in msg, msg
    assert msg.count("guard band damaged") == 1


def test_placement_policy(be):
    """Shift 0 by default and after the policy ends; inside it dev() / out() / zeros() sit `shift` bytes past a 16-byte boundary, 8-byte
    element types never below 8, scratch() always on the boundary; `only` and `place` single buffers out by their allocation index."""
    x = np.arange(6, dtype=np.float32)
    assert [be.ptr(b) % 16 for b in (be.dev(x), be.out((3,)), be.zeros((3,)), be.scratch(5))] == [0, 0, 0, 0]
    for shift in (4, 8):
        with be.misaligned(shift):
            bufs = [be.dev(x), be.out((3,)), be.zeros((3,)), be.out((2,), np.complex64), be.dev(np.array([7], np.int64)), be.scratch(5)]
            assert [be.ptr(b) % 16 for b in bufs] == [shift, shift, shift, 8, 8, 0]
            assert be.allocations == 5                                          # (scratch() is not counted)
            assert np.array_equal(be.host(bufs[0]), x) and not be.host(bufs[2]).any() and int(be.host(bufs[4])[0]) == 7
            assert (be.host(bufs[1]).view(np.uint32) == BK.POISON_WORD).all() and (be.host(bufs[3]).view(np.uint32) == BK.POISON_WORD).all()
    with be.misaligned(4, only=1):
        assert [be.ptr(be.out((3,))) % 16 for _ in range(3)] == [0, 4, 0]
    with be.misaligned(4, place={0: 0, 2: 8}):
        assert [be.ptr(be.out((3,))) % 16 for _ in range(3)] == [0, 4, 8]
    with be.misaligned(0):
        assert be.ptr(be.out((3,))) % 16 == 0
    assert be.ptr(be.out((3,))) % 16 == 0
    be.verify()


def test_every_size_function_is_exercised_on_a_guarded_workspace():
    """The header's workspace size functions == the keys of WORKSPACE_COVERAGE; each named check asks that function for the size, puts
    exactly that many bytes in a scratch() buffer, and runs on both backends (the autouse verify() of those modules checks the guards)."""
    header = (ROOT / "include" / "cfdbench_amd.h").read_text()
    declared = set(re.findall(r"^size_t\s+(cfd_\w+)\s*\(", header, flags=re.M))
    assert declared and all(n.endswith("_bytes") or n.endswith("_bytes_ex") for n in declared), declared
    assert declared == set(K.WORKSPACE_COVERAGE), (declared - set(K.WORKSPACE_COVERAGE), set(K.WORKSPACE_COVERAGE) - declared)
    suites = {f: (ROOT / "tests" / f).read_text() for f in ("test_emul_kernels.py", "test_gpu_kernels.py")}
    callers = {"run_fno": "check_fno_vs_oracle"}  # (a helper: reached through the check that calls it)
    for fn, check in K.WORKSPACE_COVERAGE.items():
        src = inspect.getsource(getattr(K, check))
        assert f'api.size("{fn}"' in src and "be.scratch(" in src and "max(" not in src.split(f'api.size("{fn}"')[0].rsplit("\n", 1)[-1], (fn, check)
        for f, text in suites.items():
            assert f"K.{callers.get(check, check)}(" in text, (fn, check, f)
