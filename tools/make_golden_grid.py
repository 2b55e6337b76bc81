"""Reference-pinned fixtures of the FNO on grids wider than 80 columns (many-modes route whatever the mode counts): writes
tests/golden/fno_g96x100_m12.npz (forward, losses and gradient summaries of a 96 x 100 model at the default modes (12, 12), border mask) and
tests/golden/spectral_g100x120_m50x61.npz (one SpectralConv2d forward / backward at 100 x 120, modes (50, 61): every row and the Nyquist
column).  The generators are oracle/make_golden.py's and tools/make_golden_modes.py's, which run the reference's own modules on the CPU.
Run from the repository root where the reference sources are present:
    python tools/make_golden_grid.py"""
from __future__ import annotations

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from oracle.make_golden import gen_spectral  # noqa: E402
from tools.make_golden_modes import gen_fno_modes  # noqa: E402

if __name__ == "__main__":
    gen_fno_modes("fno_g96x100_m12", 101, 102, 1, 8, 2, 96, 100, 12, 12)
    gen_spectral("spectral_g100x120_m50x61", 103, 1, 3, 2, 100, 120, 50, 61)
