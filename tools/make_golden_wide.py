"""Reference-pinned fixtures of the FNO's wide-channel route (hidden 64): writes tests/golden/fno_w64_64x64.npz (forward, losses and
gradient summaries of a width-64 model) and tests/golden/rollout_w64_66x65.npz (a five-step rollout) through oracle/make_golden.py's
generators, which run the reference's own modules on the CPU.  Run from the repository root where the reference sources are present:
    python tools/make_golden_wide.py"""
from __future__ import annotations

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from oracle.make_golden import gen_fno, gen_rollout  # noqa: E402

if __name__ == "__main__":
    gen_fno("fno_w64_64x64", 91, 92, 2, 64, 2, 64, 64, border=True, full_grads=False, gain=4.0)
    gen_rollout("rollout_w64_66x65", 93, 94, 2, 64, 2, 66, 65, steps=5, border=True)
