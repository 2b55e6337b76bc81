"""MI355X: the table of tests/align_checks.py on the shipped library -- every check on buffers shifted by 4 and by 8 bytes, and every
buffer of a check shifted alone (a gate that forgets one of its pointers), must hold the tolerance against the fp64 oracle that the
check's own test uses; the placements include/cfdbench_amd.h ("Alignment") lets an entry point refuse are refused with
CFD_ERR_UNSUPPORTED before anything is written.  The CPU twin (tests/test_emul_alignment.py) runs the same rows under
-fsanitize=alignment; a row runs here only once it is green and report-free there."""
import numpy as np
import pytest

from tests import align_checks as A
from tests import backends as BK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return BK.TorchBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    yield
    be.verify()


def test_shifted_payloads_sit_where_the_policy_says(be):
    """The same placement as on the emulator backend (tests/test_emul_hostile_memory.py): pointer = shift modulo 16, guard bands around
    the payload at its place, a write 4 bytes in front of a shifted payload is caught."""
    x = np.arange(6, dtype=np.float32)
    assert [be.ptr(b) % 16 for b in (be.dev(x), be.out((3,)), be.zeros((3,)), be.scratch(5))] == [0, 0, 0, 0]
    for shift in (4, 8):
        with be.misaligned(shift):
            bufs = [be.dev(x), be.out((3,)), be.zeros((3,)), be.out((2,), np.complex64), be.dev(np.array([7], np.int64)), be.scratch(5)]
            assert [be.ptr(b) % 16 for b in bufs] == [shift, shift, shift, 8, 8, 0]
            assert be.allocations == 5
            assert np.array_equal(be.host(bufs[0]), x) and not be.host(bufs[2]).any() and int(be.host(bufs[4])[0]) == 7
            assert (be.host(bufs[1]).view(np.uint32) == BK.POISON_WORD).all() and (be.host(bufs[3]).view(np.uint32) == BK.POISON_WORD).all()
    with be.misaligned(4, only=1):
        assert [be.ptr(be.out((3,))) % 16 for _ in range(3)] == [0, 4, 0]
    be.verify()
    with be.misaligned(4):
        y = be.out((9,))
    be.guard_front(y)[-4:] = 0  # the four bytes in front of the payload (memory of this test's own allocation)
    with pytest.raises(AssertionError, match=r"out shape=\(9,\) dtype=float32 shift=4: front guard band damaged, first at byte 4096 of 4100, 4 byte"):
        be.verify()
    assert be.ptr(y) % 16 == 4


@pytest.mark.parametrize("row,placement", [(r, p) for r in A.ROWS for p in A.placements(r, False)], ids=lambda v: getattr(v, "id", v))
def test_row_on_misaligned_buffers(be, row, placement):
    A.run_row(be, row, placement)
