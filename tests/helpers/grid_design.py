"""What the injection-grid tests share (tests/test_inject_grid_cpu.py, tests/test_gpu_inject_grid.py): the list of
injections, grid_index.h's byte count per injection restated, and the design whose middle entry ends its components."""
import numpy as np

from helpers import sysrem_ref as sref

# (trial, scale) of a 3-trial table: a duplicate and a scale of 0
LIST = [(1, 0.7), (0, 1.3), (1, 0.7), (2, 0.0), (2, -0.5)]
FLAGS = 17                                        # kGrFlags: kSyMaxComp + 1


def injection_bytes(n_exp, n_pix, n_cols, n_tap, recover):
    """gr_injection_bytes: D, out, the injected model, r, w (pitched), a, part, U, Fj, the flags and, for a recovery, W."""
    tiles = (n_pix + sref.TILE - 1) // sref.TILE
    n = n_exp * n_pix
    d = 3 * n + 2 * n_exp * tiles * sref.TILE + n_exp + 2 * n_exp * tiles + n_exp * n_cols + n_exp * n_tap
    if recover:
        d += n_cols * n
    return 8 * d + 4 * FLAGS


def overflow_design():
    """(design, points): test_gpu_sysrem.design(7, 129) with every pixel inside the wavelength grid (each has a model,
    and the spectrum of observe_ref lies below 1 everywhere, so M - 1 < 0 at every pixel) and raw data of the order
    1e10.  At scale 1e305 the middle point's D = raw (1 + scale (M - 1)) overflows wherever raw is not NaN: no entry
    keeps a weight, every norm is 0 and every component of that injection ends at once, while its neighbours' scales
    leave D finite."""
    import test_gpu_sysrem as ts
    d = ts.design(7, 129, seed=31)
    wav = d["wav"]
    d["lam"] = np.linspace(wav[200], wav[-200], 129)
    d["raw"] = d["raw"] * 1e10
    return d, [(0, 0.7), (1, 1e305), (2, -0.5)]
