"""ctypes binding of libprom_hip.so (C-ABI declared in include/prom_hip.h).

The library is built in-tree for gfx950 (``python -m prometheus_amd.build`` or
``__graft_entry__.build()``).  There is no CPU fallback: if the library or a GPU is
missing, every compute call raises ``NativeUnavailable``.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Dict, Optional, Sequence

import numpy as np

LIB_NAME = "libprom_hip.so"
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)

PROM_OK = 0
STATUS = {-1: "PROM_E_ARG", -2: "PROM_E_HIP", -3: "PROM_E_NOMEM", -4: "PROM_E_STATE"}

DENSITY_BAROMETRIC = 1
DENSITY_HYDROSTATIC = 2
DENSITY_POWERLAW = 3
DENSITY_TORUS = 4
DENSITY_TABULATED = 5
DENSITY_GRIDDED = 6

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class NativeUnavailable(RuntimeError):
    """The HIP library is not built/loadable or no GPU is visible."""


class NativeError(RuntimeError):
    pass


class DensityModel(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("p", C.c_double * 8)]


class Constituent(C.Structure):
    _fields_ = [("table_id", C.c_int32), ("is_molecule", C.c_int32), ("chi", C.c_double)]


class Scenario(C.Structure):
    _fields_ = [("density", DensityModel), ("body_x", _dp), ("body_y", _dp), ("shift", _dp),
                ("n_tabulated", _dp), ("T", C.c_double), ("n_constituents", C.c_int32),
                ("reserved", C.c_int32), ("constituents", C.POINTER(Constituent))]


class TransitProblem(C.Structure):
    _fields_ = [("n_wav", C.c_int64), ("wavelength", _dp), ("n_pr", C.c_int32), ("n_orb", C.c_int32),
                ("chord_y", _dp), ("chord_z", _dp), ("chord_fout", _dp), ("n_x", C.c_int32),
                ("n_scenarios", C.c_int32), ("x", _dp), ("delta_x", C.c_double), ("planet_y", _dp),
                ("planet_R", C.c_double), ("n_moons", C.c_int32), ("reserved", C.c_int32),
                ("moon_y", _dp), ("moon_R", _dp), ("scenarios", C.POINTER(Scenario)),
                ("cull_tau", C.c_double), ("options", C.c_int32), ("reserved2", C.c_int32),
                ("k_B", C.c_double), ("has_star", C.c_int32), ("star_table", C.c_int32),
                ("chord_rho", _dp), ("chord_clv", _dp), ("chord_star_shift", _dp)]


ABI_VERSION = 6
# prom_kernel_id order (prom_hip.h): the keys of Device.transit_kernel_ms
KERNEL_IDS = ("columns", "sigma", "order", "windows", "tau", "tc_build", "sigma_tc")
# prom_transit_stats.tau_kernel_variant // 10 -> the integration path the run took (prom_hip.h)
VARIANT_PATHS = {0: "k_tau (ocml exp, validation)", 1: "k_tau / k_tau_mol (table exp)", 2: "k_tau_w (windowed)",
                 3: "k_tau_p (planned windows)", 4: "k_tau_rm (stellar spectrum)",
                 8: "k_tc_build + k_sigma_tc (transmission curves)",
                 9: "k_tc_build + k_sigma_tw (transmission curves, target-window lookups)"}
OPT_OCML_EXP = 1
OPT_NO_MERGE = 2
OPT_NO_WINDOW = 4
OPT_DOPPLER_ROWS = 8


class TransitStats(C.Structure):
    _fields_ = [("ms_total", C.c_double), ("ms_density", C.c_double), ("ms_sigma", C.c_double),
                ("ms_tau", C.c_double), ("active_chords", C.c_int64), ("transparent_chords", C.c_int64),
                ("blocked_chords", C.c_int64), ("chord_lambda_evals", C.c_int64),
                ("tau_records", C.c_int64), ("exp_evals", C.c_int64),
                ("tau_kernel_variant", C.c_int32), ("exact_phases", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


# every exported symbol: name -> (restype, argtypes)
SIGNATURES = {
    "prom_abi_version": (C.c_int32, []),
    "prom_device_count": (C.c_int32, [_ip]),
    "prom_create": (C.c_int32, [C.c_int32, C.POINTER(C.c_void_p)]),
    "prom_destroy": (None, [C.c_void_p]),
    "prom_last_error": (C.c_char_p, [C.c_void_p]),
    "prom_synchronize": (C.c_int32, [C.c_void_p]),
    "prom_table_upload": (C.c_int32, [C.c_void_p, C.c_int64, _dp, _dp, C.c_double, _ip]),
    "prom_table_build_voigt": (C.c_int32, [C.c_void_p, C.c_int64, _dp, C.c_int32, _dp, _dp, _dp,
                                           C.c_double, C.c_double, C.c_double, _ip, _dp]),
    "prom_voigt_sigma": (C.c_int32, [C.c_void_p, C.c_int64, _dp, C.c_int32, _dp, _dp, _dp, C.c_double,
                                     C.c_double, _dp]),
    "prom_table_lookup": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, _dp, _dp]),
    "prom_table_free": (C.c_int32, [C.c_void_p, C.c_int32]),
    "prom_table_count": (C.c_int32, [C.c_void_p, _ip, _ip, C.POINTER(C.c_int64)]),
    "prom_molecular_free": (C.c_int32, [C.c_void_p, C.c_int32]),
    "prom_molecular_upload": (C.c_int32, [C.c_void_p, C.c_int32, _dp, C.c_int32, _dp, C.c_int64, _dp, _dp,
                                          C.c_double, _ip]),
    "prom_molecular_sigma": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, _dp, C.c_double,
                                         C.c_int64, _dp, _dp]),
    "prom_number_density": (C.c_int32, [C.c_void_p, C.POINTER(DensityModel), C.c_int32, _dp, C.c_int64,
                                        _dp, _dp, _dp, _dp, _dp]),
    "prom_gridded_density": (C.c_int32, [C.c_void_p, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, _dp, _dp,
                                         C.c_int64, _dp, _dp, _dp, _dp]),
    "prom_transit_set": (C.c_int32, [C.c_void_p, C.POINTER(TransitProblem)]),
    "prom_transit_run": (C.c_int32, [C.c_void_p, C.POINTER(TransitStats)]),
    "prom_transit_result": (C.c_int32, [C.c_void_p, _dp]),
    "prom_transit_columns": (C.c_int32, [C.c_void_p, _dp]),
    "prom_transit_band_stats": (C.c_int32, [C.c_void_p, C.c_int32, _dp, _dp, C.POINTER(C.c_int64), _dp]),
    "prom_transit_kernel_ms": (C.c_int32, [C.c_void_p, C.c_int32, _dp]),
    "prom_observe_set": (C.c_int32, [C.c_void_p, C.c_int32, _dp, _dp, C.c_double, C.c_int32, _dp, _dp, _dp]),
    "prom_transit_observe": (C.c_int32, [C.c_void_p, C.c_double, C.c_double, _dp, _dp, _dp, C.POINTER(C.c_int64)]),
    "prom_spectrum_observe": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, _dp, _dp, C.c_double, C.c_double, _dp,
                                          _dp, _dp, C.POINTER(C.c_int64)]),
    "prom_observe_kernel_ms": (C.c_int32, [C.c_void_p, C.c_int32, _dp]),
    "prom_vmap_set": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _dp]),
    "prom_transit_vmap": (C.c_int32, [C.c_void_p, _dp, C.POINTER(C.c_int64)]),
    "prom_spectrum_vmap": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, _dp, _dp, _dp, C.POINTER(C.c_int64)]),
    "prom_vmap_kernel_ms": (C.c_int32, [C.c_void_p, C.c_int32, _dp]),
    "prom_expose_set": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), _dp, _dp, _dp,
                                    _dp]),
    "prom_transit_expose": (C.c_int32, [C.c_void_p, _dp, C.POINTER(C.c_int64), _dp]),
    "prom_spectrum_expose": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, _dp, _dp, _dp, C.POINTER(C.c_int64), _dp]),
    "prom_expose_kernel_ms": (C.c_int32, [C.c_void_p, C.c_int32, _dp]),
    "prom_detrend_set": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _dp, _dp]),
    "prom_transit_expose_detrended": (C.c_int32, [C.c_void_p, _dp, C.POINTER(C.c_int64), _dp]),
    "prom_spectrum_expose_detrended": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, _dp, _dp, _dp,
                                                   C.POINTER(C.c_int64), _dp]),
    "prom_detrend_kernel_ms": (C.c_int32, [C.c_void_p, C.c_int32, _dp]),
    "prom_highpass_set": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      C.c_int32, _dp, C.c_int32]),
    "prom_highpass_set_median": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int32), C.c_int32, C.c_int32]),
    "prom_transit_expose_highpass": (C.c_int32, [C.c_void_p, C.c_int32, _dp, C.POINTER(C.c_int64), _dp]),
    "prom_spectrum_expose_highpass": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, _dp, _dp, C.c_int32, _dp,
                                                  C.POINTER(C.c_int64), _dp]),
    "prom_highpass_kernel_ms": (C.c_int32, [C.c_void_p, C.c_int32, _dp]),
    "prom_orders_set": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_uint8)]),
    "prom_transit_expose_orders": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _dp, C.POINTER(C.c_int64), _dp,
                                               C.POINTER(C.c_int64), _dp, _dp]),
    "prom_spectrum_expose_orders": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, _dp, _dp, C.c_int32, C.c_int32, _dp,
                                                C.POINTER(C.c_int64), _dp, C.POINTER(C.c_int64), _dp, _dp]),
    "prom_orders_kernel_ms": (C.c_int32, [C.c_void_p, C.c_int32, _dp]),
    "prom_broaden_set": (C.c_int32, [C.c_void_p, C.c_int32, C.c_double, C.c_double, _dp]),
    "prom_spectrum_broaden": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, _dp, _dp, _dp]),
    "prom_transit_broaden": (C.c_int32, [C.c_void_p]),
    "prom_transit_broadened": (C.c_int32, [C.c_void_p, _dp]),
    "prom_broaden_kernel_ms": (C.c_int32, [C.c_void_p, C.c_int32, _dp]),
    "prom_sysrem_set": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _dp]),
    "prom_sysrem_clean": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp]),
    "prom_transit_inject": (C.c_int32, [C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        _dp, _dp, _dp]),
    "prom_spectrum_inject": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, _dp, _dp, C.c_int32, C.c_double, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp]),
    "prom_sysrem_kernel_ms": (C.c_int32, [C.c_void_p, C.c_int32, _dp]),
    "prom_filter_weights": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp]),
    "prom_detrend_build": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _dp, _dp]),
    "prom_filter_kernel_ms": (C.c_int32, [C.c_void_p, C.c_int32, _dp]),
    "prom_transit_recover": (C.c_int32, [C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, _dp, C.POINTER(C.c_int64), _dp, C.POINTER(C.c_int64), _dp, _dp,
                                         _dp]),
    "prom_spectrum_recover": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, _dp, _dp, C.c_int32, C.c_double, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, C.POINTER(C.c_int64), _dp,
                                          C.POINTER(C.c_int64), _dp, _dp, _dp]),
    "prom_transit_inject_grid": (C.c_int32, [C.c_void_p, C.c_int32, _ip, _dp, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, _dp, _dp, _dp]),
    "prom_spectrum_inject_grid": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, _dp, _dp, C.c_int32, _ip, _dp,
                                              C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp]),
    "prom_transit_recover_grid": (C.c_int32, [C.c_void_p, C.c_int32, _ip, _dp, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_int32, _dp, C.POINTER(C.c_int64), _dp, _dp]),
    "prom_spectrum_recover_grid": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, _dp, _dp, C.c_int32, _ip, _dp,
                                               C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp,
                                               C.POINTER(C.c_int64), _dp, _dp]),
    "prom_sysrem_clean_orders": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp]),
    "prom_transit_inject_orders": (C.c_int32, [C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_int32, _dp, _dp, _dp]),
    "prom_spectrum_inject_orders": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, _dp, _dp, C.c_int32, C.c_double,
                                                C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp]),
    "prom_transit_inject_grid_orders": (C.c_int32, [C.c_void_p, C.c_int32, _ip, _dp, C.c_int32, C.c_int32, C.c_int32,
                                                    C.c_int32, _dp, _dp, _dp]),
    "prom_spectrum_inject_grid_orders": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, _dp, _dp, C.c_int32, _ip, _dp,
                                                     C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp]),
    "prom_filter_weights_orders": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _ip, _dp, _dp,
                                               _dp]),
    "prom_detrend_set_orders": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _dp, _dp]),
    "prom_detrend_build_orders": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _dp, _dp]),
    "prom_star_disk_flux": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _dp, _dp, _dp, C.c_double, C.c_double,
                                        C.c_int64, _dp, _dp]),
    "prom_timing_begin": (C.c_int32, [C.c_void_p]),
    "prom_timing_end": (C.c_int32, [C.c_void_p, C.c_int32, _dp, _ip]),
    "prom_timing_stride": (C.c_int32, [C.c_void_p, C.c_int32]),
    "prom_host_alloc": (C.c_int32, [C.c_int64, C.POINTER(C.c_void_p)]),
    "prom_host_free": (C.c_int32, [C.c_void_p]),
}

_lib = None
_lib_lock = threading.Lock()


def load_library(path: Optional[str] = None):
    """Load (once) and type the C-ABI library.  Raises NativeUnavailable if absent."""
    global _lib
    with _lib_lock:
        if _lib is not None and path is None:
            return _lib
        p = path or os.environ.get("PROMETHEUS_AMD_LIB", LIB_PATH)
        if not os.path.exists(p):
            raise NativeUnavailable("%s not found: build it with `python -m prometheus_amd.build` "
                                    "(hipcc --offload-arch=gfx950); there is no CPU fallback" % p)
        try:
            lib = C.CDLL(p)
        except OSError as e:  # pragma: no cover - depends on the image
            raise NativeUnavailable("cannot load %s: %s" % (p, e))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.prom_abi_version() != ABI_VERSION:
            raise NativeUnavailable("ABI version mismatch")
        if path is None:
            _lib = lib
        return lib


def device_count() -> int:
    lib = load_library()
    n = C.c_int32(0)
    lib.prom_device_count(C.byref(n))
    return int(n.value)


class _PinnedBuffer:
    """A prom_host_alloc buffer exposed to numpy; returned to the pool when the last array over it dies."""

    def __init__(self, lib, ptr: int, shape):
        self._lib, self._ptr = lib, ptr
        self.__array_interface__ = {"shape": tuple(shape), "typestr": "<f8", "data": (ptr, False), "version": 3}

    def __del__(self):  # pragma: no cover - interpreter teardown order
        try:
            self._lib.prom_host_free(C.c_void_p(self._ptr))
        except Exception:
            pass


def host_array(shape) -> Optional[np.ndarray]:
    """A float64 array of ``shape`` in page-locked memory from the library's pool (prom_host_alloc), or None
    when the pool's cap (PROM_PINNED_CAP_MB) is reached.  Device results copy into it with one DMA."""
    lib = load_library()
    n = int(np.prod(shape, dtype=np.int64)) * 8
    p = C.c_void_p()
    if lib.prom_host_alloc(n, C.byref(p)) != PROM_OK or not p.value:
        return None
    return np.asarray(_PinnedBuffer(lib, p.value, shape))


_pinned_usable: Optional[bool] = None


def pinned_copy(a) -> np.ndarray:
    """``a`` as a C-contiguous float64 array in the pinned pool (inputs re-sent on every call, such as the
    wavelength grid, then reach the device in one DMA), or an ordinary copy without a GPU or past the cap."""
    global _pinned_usable
    a = np.asarray(a, dtype=np.float64)
    if _pinned_usable is None:
        try:
            _pinned_usable = device_count() > 0
        except NativeUnavailable:
            _pinned_usable = False
    out = host_array(a.shape) if _pinned_usable and a.size else None
    if out is None:
        return np.array(a, dtype=np.float64, order="C")
    out[...] = a
    return out


def _d(a: np.ndarray):
    return a.ctypes.data_as(_dp)


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def _spectrum(wav, R, who: str):
    """The arguments of Device.``who``: the grid wav [n_wav] and R [n_orb][n_wav] as contiguous float64 arrays."""
    wav, R = _f64(wav), _f64(R)
    if R.ndim != 2 or wav.ndim != 1 or R.shape[1] != len(wav):
        raise ValueError("%s: R must be [n_orb][n_wav]" % who)
    return wav, R


class Device:
    """One prom_ctx (one GPU).  Not thread-safe; use one Device per host thread."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        n = device_count()
        if n == 0:
            raise NativeUnavailable("no HIP device visible (libprom_hip needs an MI355X / gfx950 GPU)")
        h = C.c_void_p()
        st = self.lib.prom_create(int(device), C.byref(h))
        if st != PROM_OK:
            raise NativeUnavailable("prom_create(%d) failed with %s" % (device, STATUS.get(st, st)))
        self.h = h
        self.device = int(device)
        self._keep = []
        # tables whose host objects were collected: freed at the next table or problem upload (a
        # finalizer may run while another thread is inside a call on this context)
        self._pending_free: list = []
        # the observation resident on the context: (n_orb, n_pix) and the caller's key (None: none)
        self._obs_shape = None
        self._obs_key = None
        self._vm_shape = None
        self._vm_key = None
        self._ex_shape = None
        self._ex_key = None
        self._dt_key = None
        self._hp_key = None
        self._od_key = None
        self._od_n_seg = 0
        self._br_key = None
        self._sy_key = None
        self._dt_per_order = False   # the resident filter is a per-order one (orders_set then drops it)

    def close(self):
        if getattr(self, "h", None):
            self.lib.prom_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int, what: str):
        if st != PROM_OK:
            msg = self.lib.prom_last_error(self.h)
            raise NativeError("%s: %s (%s)" % (what, STATUS.get(st, st), msg.decode() if msg else ""))

    def synchronize(self):
        self._check(self.lib.prom_synchronize(self.h), "prom_synchronize")

    # ---- tables -----------------------------------------------------------------------
    def release_later(self, molecular: bool, table_id: int) -> None:
        """Queue a table for prom_table_free / prom_molecular_free (safe from finalizers)."""
        self._pending_free.append((bool(molecular), int(table_id)))

    def _drain_frees(self) -> None:
        while self._pending_free:
            mol, tid = self._pending_free.pop()
            self.table_free(tid, molecular=mol)

    def table_free(self, table_id: int, molecular: bool = False) -> None:
        fn = self.lib.prom_molecular_free if molecular else self.lib.prom_table_free
        self._check(fn(self.h, int(table_id)), "prom_molecular_free" if molecular else "prom_table_free")

    def table_count(self):
        """(live atomic tables, live molecular tables, device bytes they hold)."""
        a, m, b = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        self._check(self.lib.prom_table_count(self.h, C.byref(a), C.byref(m), C.byref(b)), "prom_table_count")
        return int(a.value), int(m.value), int(b.value)

    def table_upload(self, x, y, offset: float) -> int:
        self._drain_frees()
        x, y = _f64(x), _f64(y)
        tid = C.c_int32(-1)
        self._check(self.lib.prom_table_upload(self.h, len(x), _d(x), _d(y), float(offset), C.byref(tid)),
                    "prom_table_upload")
        return int(tid.value)

    def table_build_voigt(self, x, line_w, line_g, line_coef, sigma_v, c_light, offset, want_host=True):
        self._drain_frees()
        x, lw, lg, lc = _f64(x), _f64(line_w), _f64(line_g), _f64(line_coef)
        out = np.empty_like(x) if want_host else None
        tid = C.c_int32(-1)
        self._check(self.lib.prom_table_build_voigt(self.h, len(x), _d(x), len(lw), _d(lw), _d(lg), _d(lc),
                                                    float(sigma_v), float(c_light), float(offset), C.byref(tid),
                                                    _d(out) if out is not None else None),
                    "prom_table_build_voigt")
        return int(tid.value), out

    def voigt_sigma(self, x, line_w, line_g, line_coef, sigma_v, c_light) -> np.ndarray:
        x, lw, lg, lc = _f64(x), _f64(line_w), _f64(line_g), _f64(line_coef)
        out = np.empty_like(x)
        self._check(self.lib.prom_voigt_sigma(self.h, x.size, _d(x), len(lw), _d(lw), _d(lg), _d(lc),
                                              float(sigma_v), float(c_light), _d(out)), "prom_voigt_sigma")
        return out

    def table_lookup(self, table_id: int, targets) -> np.ndarray:
        t = _f64(targets)
        out = np.empty_like(t)
        self._check(self.lib.prom_table_lookup(self.h, int(table_id), t.size, _d(t), _d(out)),
                    "prom_table_lookup")
        return out

    # ---- molecular ----------------------------------------------------------------------
    def molecular_upload(self, P, T, W, V, offset) -> int:
        self._drain_frees()
        P, T, W, V = _f64(P), _f64(T), _f64(W), _f64(V)
        assert V.shape == (len(P), len(T), len(W))
        tid = C.c_int32(-1)
        self._check(self.lib.prom_molecular_upload(self.h, len(P), _d(P), len(T), _d(T), len(W), _d(W), _d(V),
                                                   float(offset), C.byref(tid)), "prom_molecular_upload")
        return int(tid.value)

    def molecular_sigma(self, table_id, P, T, wav) -> np.ndarray:
        P, wav = _f64(P), _f64(wav)
        nc, nx = P.shape
        assert wav.shape[0] == nc
        nw = wav.shape[1]
        out = np.empty((nc, nx, nw))
        self._check(self.lib.prom_molecular_sigma(self.h, int(table_id), nc, nx, _d(P), float(T), nw, _d(wav),
                                                  _d(out)), "prom_molecular_sigma")
        return out

    # ---- density ------------------------------------------------------------------------
    def number_density(self, kind: int, params: Sequence[float], x, y, z, bx, by) -> np.ndarray:
        m = DensityModel()
        m.kind = int(kind)
        for i, v in enumerate(params):
            m.p[i] = float(v)
        x, y, z, bx, by = _f64(x), _f64(y), _f64(z), _f64(bx), _f64(by)
        out = np.empty((len(y), len(x)))
        self._check(self.lib.prom_number_density(self.h, C.byref(m), len(x), _d(x), len(y), _d(y), _d(z), _d(bx),
                                                 _d(by), _d(out)), "prom_number_density")
        return out

    def gridded_density(self, gx, gy, gz, values, px, py, pz) -> np.ndarray:
        """prom_gridded_density: scipy RegularGridInterpolator (linear) of values on (gx, gy, gz) at the
        points (px, py, pz); NaN outside the grid."""
        gx, gy, gz = _f64(gx), _f64(gy), _f64(gz)
        v = _f64(values)
        if v.shape != (len(gx), len(gy), len(gz)):
            raise ValueError("values must have shape (len(gx), len(gy), len(gz))")
        px, py, pz = np.broadcast_arrays(_f64(px), _f64(py), _f64(pz))
        px, py, pz = _f64(px), _f64(py), _f64(pz)
        out = np.empty(px.shape)
        self._check(self.lib.prom_gridded_density(self.h, len(gx), _d(gx), len(gy), _d(gy), len(gz), _d(gz), _d(v),
                                                  px.size, _d(px), _d(py), _d(pz), _d(out)), "prom_gridded_density")
        return out

    # ---- transit ------------------------------------------------------------------------
    def transit_set(self, prob: "TransitInputs"):
        self._drain_frees()
        self._keep = prob.keepalive
        self._check(self.lib.prom_transit_set(self.h, C.byref(prob.struct)), "prom_transit_set")
        self._shape = (prob.struct.n_orb, prob.struct.n_wav)
        if self._obs_shape is not None and self._obs_shape[0] != prob.struct.n_orb:
            self._obs_shape = self._obs_key = None   # the library dropped the observation
            self._vm_shape = self._vm_key = None     # ... and the trial table with it
            self._ex_shape = self._ex_key = None     # ... and the exposure table
            self._dt_key = None                      # ... with its filter
            self._hp_key = None                      # ... and its high-pass
            self._od_key = None                      # ... and its orders
            self._sy_key = None                      # ... and its raw exposures
        self._n_atoms = prob.n_atoms
        self._n_pr = prob.struct.n_pr

    def transit_run(self, stats: bool = False):
        st = TransitStats() if stats else None
        self._check(self.lib.prom_transit_run(self.h, C.byref(st) if st is not None else None), "prom_transit_run")
        return st.as_dict() if st is not None else None

    def transit_result(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        """R of the last run, [n_orb, n_wav]; ``out``: a C-contiguous float64 array of that shape to fill."""
        if out is None:
            out = np.empty(self._shape)
        elif out.shape != self._shape or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("transit_result: out must be a C-contiguous float64 array of shape %s" % (self._shape,))
        self._check(self.lib.prom_transit_result(self.h, _d(out)), "prom_transit_result")
        return out

    def timing_begin(self, stride: int = 1):
        """Start a timing window; events ride on every ``stride``-th run's tau dispatch."""
        self._check(self.lib.prom_timing_stride(self.h, int(stride)), "prom_timing_stride")
        self._check(self.lib.prom_timing_begin(self.h), "prom_timing_begin")

    def timing_end(self, max_runs: int = 4096) -> np.ndarray:
        """ms[run] = (NaN, NaN, tau_events, tau_device) of every timed run since timing_begin: the HIP
        event interval from the ordering kernel's completion to the tau kernel's, and the tau kernel's
        span on the device clock (first workgroup start -> last workgroup end; NaN unless k_tau_p)."""
        ms = np.zeros((max_runs, 4))
        n = C.c_int32(0)
        self._check(self.lib.prom_timing_end(self.h, max_runs, _d(ms), C.byref(n)), "prom_timing_end")
        return ms[:min(int(n.value), max_runs)]

    KERNEL_IDS = KERNEL_IDS

    def transit_kernel_ms(self, n_runs: int = 20) -> dict:
        """prom_transit_kernel_ms: mean device duration [ms] of each kernel of the current problem over
        n_runs serialized runs (one slot; dispatch-packet events), None for kernels the path does not launch."""
        ms = np.empty(len(self.KERNEL_IDS))
        self._check(self.lib.prom_transit_kernel_ms(self.h, int(n_runs), _d(ms)), "prom_transit_kernel_ms")
        return {k: (float(v) if np.isfinite(v) else None) for k, v in zip(self.KERNEL_IDS, ms)}

    def transit_columns(self) -> np.ndarray:
        out = np.empty((self._n_atoms, self._shape[0], self._n_pr))
        self._check(self.lib.prom_transit_columns(self.h, _d(out)), "prom_transit_columns")
        return out

    def transit_band_stats(self, bounds):
        """(sum, count, max) per phase of the last run's R over the band windows bounds[o][b] = (lo, hi)."""
        b = _f64(bounds)
        n_orb = self._shape[0]
        if b.ndim != 3 or b.shape[0] != n_orb or b.shape[2] != 2:
            raise ValueError("bounds must be [n_orb][n_bands][2]")
        s, c, m = np.empty(n_orb), np.empty(n_orb, dtype=np.int64), np.empty(n_orb)
        self._check(self.lib.prom_transit_band_stats(self.h, b.shape[1], _d(b), _d(s),
                                                     c.ctypes.data_as(C.POINTER(C.c_int64)), _d(m)),
                    "prom_transit_band_stats")
        return s, c, m

    # ---- observation (prom_hip.h "observation of a spectrum on the device") -------------------
    def observe_set(self, lam, sig, k: float, n_orb: int, f=None, data=None, ivar=None, key=None) -> None:
        """prom_observe_set: pixel centres (non-decreasing) and widths [n_pix], truncation k, the phases' frame
        factors f [n_orb] (None: all 1) and data / ivar [n_orb][n_pix] (None: no chi-square).  ``key``: any value
        the caller keeps in ``observe_key`` to skip a later upload of the same observation."""
        lam, sig = _f64(lam), _f64(sig)
        if lam.ndim != 1 or sig.shape != lam.shape:
            raise ValueError("observe_set: lam and sig must be 1-D arrays of one length")
        n_pix, n_orb = len(lam), int(n_orb)
        f = None if f is None else _f64(f)
        if f is not None and f.shape != (n_orb,):
            raise ValueError("observe_set: f must be [n_orb]")
        if (data is None) != (ivar is None):
            raise ValueError("observe_set: data and ivar come together")
        if data is not None:
            data, ivar = _f64(data), _f64(ivar)
            if data.shape != (n_orb, n_pix) or ivar.shape != (n_orb, n_pix):
                raise ValueError("observe_set: data and ivar must be [n_orb][n_pix]")
        self._obs_shape = self._obs_key = None
        self._vm_shape = self._vm_key = None   # the library drops the trial table with the observation it was set for
        self._ex_shape = self._ex_key = None   # ... and the exposure table
        self._dt_key = None                    # ... with its filter
        self._hp_key = None                    # ... and its high-pass
        self._od_key = None                    # ... and its orders
        self._sy_key = None                    # ... and its raw exposures
        self._check(self.lib.prom_observe_set(self.h, n_pix, _d(lam), _d(sig), float(k), n_orb,
                                              _d(f) if f is not None else None,
                                              _d(data) if data is not None else None,
                                              _d(ivar) if ivar is not None else None), "prom_observe_set")
        self._obs_shape = (n_orb, n_pix)
        self._obs_key = key

    @property
    def observe_key(self):
        """The ``key`` of the observation resident on the context (None: none, or set without a key)."""
        return self._obs_key

    def _observe_outputs(self, partials: bool, chi2: bool):
        shape = self._obs_shape or (0, 0)
        num = den = None
        if partials:
            # large partial sums land in page-locked memory from the library's pool (one DMA each at the link rate)
            big = shape[0] * shape[1] * 8 >= (1 << 20)
            num = host_array(shape) if big else None
            den = host_array(shape) if big else None
            num = np.zeros(shape) if num is None else num
            den = np.zeros(shape) if den is None else den
        c2 = np.zeros(shape[0]) if chi2 else None
        nu = np.zeros(shape[0], dtype=np.int64) if chi2 else None
        ptr = (_d(num) if partials else None, _d(den) if partials else None, _d(c2) if chi2 else None,
               nu.ctypes.data_as(C.POINTER(C.c_int64)) if chi2 else None)
        return (num, den, c2, nu), ptr

    def transit_observe(self, edge_lo: float = np.nan, edge_hi: float = np.nan, partials: bool = True,
                        chi2: bool = False):
        """prom_transit_observe over the last run's R: (num, den, chi2, n_used), None for what was not asked."""
        out, ptr = self._observe_outputs(partials, chi2)
        self._check(self.lib.prom_transit_observe(self.h, float(edge_lo), float(edge_hi), *ptr),
                    "prom_transit_observe")
        return out

    def spectrum_observe(self, wav, R, edge_lo: float = np.nan, edge_hi: float = np.nan, partials: bool = True,
                         chi2: bool = False):
        """prom_spectrum_observe of R[n_orb][n_wav] on the ascending grid wav: (num, den, chi2, n_used)."""
        wav, R = _spectrum(wav, R, "spectrum_observe")
        out, ptr = self._observe_outputs(partials, chi2)
        self._check(self.lib.prom_spectrum_observe(self.h, R.shape[0], len(wav), _d(wav), _d(R), float(edge_lo),
                                                   float(edge_hi), *ptr), "prom_spectrum_observe")
        return out

    def observe_kernel_ms(self, n_runs: int = 20) -> float:
        """prom_observe_kernel_ms: mean device duration [ms] of k_observe for the last observe call's launch."""
        ms = C.c_double(0.0)
        self._check(self.lib.prom_observe_kernel_ms(self.h, int(n_runs), C.byref(ms)), "prom_observe_kernel_ms")
        return float(ms.value)

    # ---- velocity maps (prom_hip.h "velocity maps on the device") -----------------------------
    def vmap_set(self, F, key=None) -> None:
        """prom_vmap_set: the trial table F[n_orb][n_trial] of frame factors (finite, > 0) for the resident
        observation, which must hold data.  ``key``: any value the caller keeps in ``vmap_key`` to skip a later upload
        of the same table."""
        F = _f64(F)
        if F.ndim != 2:
            raise ValueError("vmap_set: F must be [n_orb][n_trial]")
        self._vm_shape = self._vm_key = None
        self._check(self.lib.prom_vmap_set(self.h, F.shape[0], F.shape[1], _d(F)), "prom_vmap_set")
        self._vm_shape = F.shape
        self._vm_key = key

    @property
    def vmap_key(self):
        """The ``key`` of the trial table resident on the context (None: none, or set without a key)."""
        return self._vm_key

    def _vmap_outputs(self):
        shape = self._vm_shape or (0, 0)
        mom = np.zeros(shape + (7,))
        nu = np.zeros(shape, dtype=np.int64)
        return mom, nu

    def transit_vmap(self):
        """prom_transit_vmap over the last run's R: (moments [n_orb][n_trial][7], n_used [n_orb][n_trial])."""
        mom, nu = self._vmap_outputs()
        self._check(self.lib.prom_transit_vmap(self.h, _d(mom), nu.ctypes.data_as(C.POINTER(C.c_int64))),
                    "prom_transit_vmap")
        return mom, nu

    def spectrum_vmap(self, wav, R):
        """prom_spectrum_vmap of R[n_orb][n_wav] on the ascending grid wav: (moments, n_used)."""
        wav, R = _spectrum(wav, R, "spectrum_vmap")
        mom, nu = self._vmap_outputs()
        self._check(self.lib.prom_spectrum_vmap(self.h, R.shape[0], len(wav), _d(wav), _d(R), _d(mom),
                                                nu.ctypes.data_as(C.POINTER(C.c_int64))), "prom_spectrum_vmap")
        return mom, nu

    def vmap_kernel_ms(self, n_runs: int = 20) -> float:
        """prom_vmap_kernel_ms: mean device duration [ms] of k_vmap for the last map call's launch."""
        ms = C.c_double(0.0)
        self._check(self.lib.prom_vmap_kernel_ms(self.h, int(n_runs), C.byref(ms)), "prom_vmap_kernel_ms")
        return float(ms.value)

    # ---- exposures (prom_hip.h "exposures on the device") --------------------------------------
    def expose_set(self, rows, weights, factors, data, ivar, key=None) -> None:
        """prom_expose_set: the exposure table for the resident observation's pixels: rows [n_exp][n_tap] (int, in
        [0, n_orb)), weights [n_exp][n_tap] (finite, >= 0), factors [n_exp][n_trial][n_tap] (finite, > 0), data and
        ivar [n_exp][n_pix] in the device's pixel order.  ``key``: any value the caller keeps in ``expose_key`` to
        skip a later upload of the same table."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        a, F, data, ivar = _f64(weights), _f64(factors), _f64(data), _f64(ivar)
        if rows.ndim != 2 or a.shape != rows.shape:
            raise ValueError("expose_set: rows and weights must be [n_exp][n_tap]")
        n_exp, n_tap = rows.shape
        if F.ndim != 3 or F.shape[0] != n_exp or F.shape[2] != n_tap:
            raise ValueError("expose_set: factors must be [n_exp][n_trial][n_tap]")
        n_pix = (self._obs_shape or (0, 0))[1]
        if data.shape != (n_exp, n_pix) or ivar.shape != (n_exp, n_pix):
            raise ValueError("expose_set: data and ivar must be [n_exp][n_pix] of the resident observation")
        self._ex_shape = self._ex_key = None
        self._dt_key = None   # the library drops the filter with the table it was set for
        self._hp_key = None   # ... and the high-pass
        self._od_key = None   # ... and the orders
        self._sy_key = None   # ... and the raw exposures of the injections
        self._check(self.lib.prom_expose_set(self.h, n_exp, F.shape[1], n_tap, rows.ctypes.data_as(C.POINTER(C.c_int32)),
                                             _d(a), _d(F), _d(data), _d(ivar)), "prom_expose_set")
        self._ex_shape = (n_exp, F.shape[1], n_pix)
        self._ex_key = key

    @property
    def expose_key(self):
        """The ``key`` of the exposure table resident on the context (None: none, or set without a key)."""
        return self._ex_key

    def _expose_outputs(self, moments: bool, model: bool):
        n_exp, n_trial, n_pix = self._ex_shape or (0, 0, 0)
        mom = np.zeros((n_exp, n_trial, 7)) if moments else None
        nu = np.zeros((n_exp, n_trial), dtype=np.int64) if moments else None
        mod = None
        if model:
            # NaN: what a table without pixels leaves (the library writes nothing then)
            mod = np.full((n_exp, n_trial, n_pix), np.nan)
        ptr = (_d(mom) if moments else None, nu.ctypes.data_as(C.POINTER(C.c_int64)) if moments else None,
               _d(mod) if model else None)
        return (mom, nu, mod), ptr

    def transit_expose(self, moments: bool = True, model: bool = False):
        """prom_transit_expose over the last run's R: (moments [n_exp][n_trial][7], n_used [n_exp][n_trial], model
        [n_exp][n_trial][n_pix]), None for what was not asked."""
        out, ptr = self._expose_outputs(moments, model)
        self._check(self.lib.prom_transit_expose(self.h, *ptr), "prom_transit_expose")
        return out

    def spectrum_expose(self, wav, R, moments: bool = True, model: bool = False):
        """prom_spectrum_expose of R[n_orb][n_wav] on the ascending grid wav: (moments, n_used, model)."""
        wav, R = _spectrum(wav, R, "spectrum_expose")
        out, ptr = self._expose_outputs(moments, model)
        self._check(self.lib.prom_spectrum_expose(self.h, R.shape[0], len(wav), _d(wav), _d(R), *ptr),
                    "prom_spectrum_expose")
        return out

    def expose_kernel_ms(self, n_runs: int = 20) -> float:
        """prom_expose_kernel_ms: mean device duration [ms] of k_expose for the last expose call's launch."""
        ms = C.c_double(0.0)
        self._check(self.lib.prom_expose_kernel_ms(self.h, int(n_runs), C.byref(ms)), "prom_expose_kernel_ms")
        return float(ms.value)

    # ---- detrended exposures (prom_hip.h "detrended exposures on the device") ------------------
    def detrend_set(self, U, W, key=None) -> None:
        """prom_detrend_set: the filter of the resident exposure table: U [n_exp][n_comp] and W
        [n_comp][n_exp][n_pix] in the device's pixel order, both finite, 1 <= n_comp <= 16.  ``key``: any value the
        caller keeps in ``detrend_key`` to skip a later upload of the same filter."""
        U, W = _f64(U), _f64(W)
        if U.ndim != 2:
            raise ValueError("detrend_set: U must be [n_exp][n_comp]")
        n_exp, n_comp = U.shape
        n_pix = (self._ex_shape or (0, 0, 0))[2]
        if self._ex_shape is not None and W.shape != (n_comp, n_exp, n_pix):
            raise ValueError("detrend_set: W must be [n_comp][n_exp][n_pix] of the resident exposure table")
        self._dt_key = None
        self._check(self.lib.prom_detrend_set(self.h, n_exp, n_comp, _d(U), _d(W)), "prom_detrend_set")
        self._dt_key = key
        self._dt_per_order = False

    @property
    def detrend_key(self):
        """The ``key`` of the filter resident on the context (None: none, or set without a key)."""
        return self._dt_key

    def transit_expose_detrended(self, moments: bool = True, model: bool = False):
        """prom_transit_expose_detrended over the last run's R: (moments [n_exp][n_trial][7], n_used
        [n_exp][n_trial], filtered model [n_exp][n_trial][n_pix]), None for what was not asked."""
        out, ptr = self._expose_outputs(moments, model)
        self._check(self.lib.prom_transit_expose_detrended(self.h, *ptr), "prom_transit_expose_detrended")
        return out

    def spectrum_expose_detrended(self, wav, R, moments: bool = True, model: bool = False):
        """prom_spectrum_expose_detrended of R[n_orb][n_wav] on the ascending grid wav: (moments, n_used, model)."""
        wav, R = _spectrum(wav, R, "spectrum_expose_detrended")
        out, ptr = self._expose_outputs(moments, model)
        self._check(self.lib.prom_spectrum_expose_detrended(self.h, R.shape[0], len(wav), _d(wav), _d(R), *ptr),
                    "prom_spectrum_expose_detrended")
        return out

    def detrend_kernel_ms(self, n_runs: int = 20):
        """prom_detrend_kernel_ms: mean device durations [ms] of (k_detrend, k_model_moments) for the last detrended
        call."""
        ms = (C.c_double * 2)(0.0, 0.0)
        self._check(self.lib.prom_detrend_kernel_ms(self.h, int(n_runs), ms), "prom_detrend_kernel_ms")
        return float(ms[0]), float(ms[1])

    # ---- high-pass filtered exposures (prom_hip.h "high-pass filtered exposures on the device") ----
    def highpass_set(self, seg_first, perm, g, mode: int = 0, key=None) -> None:
        """prom_highpass_set: the high-pass of the resident exposure table: the segments seg_first [n_seg + 1] and perm
        [n_pix] (int32; position i of segment s is the device pixel perm[seg_first[s] + i]), the taps g
        [half_width + 1] (finite, >= 0, g[0] > 0, half_width <= 512) and mode (0 subtracts, 1 divides).  ``key``: any
        value the caller keeps in ``highpass_key`` to skip a later upload of the same high-pass."""
        seg = np.ascontiguousarray(seg_first, dtype=np.int32)
        pm = np.ascontiguousarray(perm, dtype=np.int32)
        g = _f64(g)
        if seg.ndim != 1 or len(seg) < 2 or pm.ndim != 1 or g.ndim != 1 or len(g) < 1:
            raise ValueError("highpass_set: seg_first must be [n_seg + 1], perm [n_pix] and g [half_width + 1]")
        self._hp_key = None
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.prom_highpass_set(self.h, len(pm), len(seg) - 1, seg.ctypes.data_as(ip),
                                               pm.ctypes.data_as(ip), len(g) - 1, _d(g), int(mode)),
                    "prom_highpass_set")
        self._hp_key = key

    def highpass_set_median(self, seg_first, perm, half_width: int, mode: int = 0, key=None) -> None:
        """prom_highpass_set_median: a running median over half_width (0 .. 512) positions either side as the high-pass
        of the resident exposure table, in the place of any set before; the segments, mode and ``key`` as for
        highpass_set."""
        seg = np.ascontiguousarray(seg_first, dtype=np.int32)
        pm = np.ascontiguousarray(perm, dtype=np.int32)
        if seg.ndim != 1 or len(seg) < 2 or pm.ndim != 1:
            raise ValueError("highpass_set_median: seg_first must be [n_seg + 1] and perm [n_pix]")
        self._hp_key = None
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.prom_highpass_set_median(self.h, len(pm), len(seg) - 1, seg.ctypes.data_as(ip),
                                                      pm.ctypes.data_as(ip), int(half_width), int(mode)),
                    "prom_highpass_set_median")
        self._hp_key = key

    @property
    def highpass_key(self):
        """The ``key`` of the high-pass resident on the context (None: none, or set without a key)."""
        return self._hp_key

    def transit_expose_highpass(self, detrend: bool = False, moments: bool = True, model: bool = False):
        """prom_transit_expose_highpass over the last run's R: (moments [n_exp][n_trial][7], n_used [n_exp][n_trial],
        final model [n_exp][n_trial][n_pix]), None for what was not asked.  ``detrend``: the resident filter of
        detrend_set runs after the high-pass."""
        out, ptr = self._expose_outputs(moments, model)
        self._check(self.lib.prom_transit_expose_highpass(self.h, int(detrend), *ptr), "prom_transit_expose_highpass")
        return out

    def spectrum_expose_highpass(self, wav, R, detrend: bool = False, moments: bool = True, model: bool = False):
        """prom_spectrum_expose_highpass of R[n_orb][n_wav] on the ascending grid wav: (moments, n_used, model)."""
        wav, R = _spectrum(wav, R, "spectrum_expose_highpass")
        out, ptr = self._expose_outputs(moments, model)
        self._check(self.lib.prom_spectrum_expose_highpass(self.h, R.shape[0], len(wav), _d(wav), _d(R), int(detrend),
                                                           *ptr), "prom_spectrum_expose_highpass")
        return out

    def highpass_kernel_ms(self, n_runs: int = 20) -> float:
        """prom_highpass_kernel_ms: mean device duration [ms] of k_highpass (k_median when a median is resident) over
        the whole table for the last high-pass call."""
        ms = C.c_double(0.0)
        self._check(self.lib.prom_highpass_kernel_ms(self.h, int(n_runs), C.byref(ms)), "prom_highpass_kernel_ms")
        return float(ms.value)

    # ---- per-order moments (prom_hip.h "per-order moments on the device") ----
    def orders_set(self, seg_first, perm, keep=None, key=None) -> None:
        """prom_orders_set: the orders of the resident exposure table: seg_first [n_seg + 1] and perm [n_pix] (int32;
        position i of order s is the device pixel perm[seg_first[s] + i]) and keep [n_seg] (0 or 1; None: every order).
        ``key``: any value the caller keeps in ``orders_key`` to skip a later upload of the same orders."""
        seg = np.ascontiguousarray(seg_first, dtype=np.int32)
        pm = np.ascontiguousarray(perm, dtype=np.int32)
        if seg.ndim != 1 or len(seg) < 2 or pm.ndim != 1:
            raise ValueError("orders_set: seg_first must be [n_seg + 1] and perm [n_pix]")
        kp = np.ones(len(seg) - 1, dtype=np.uint8) if keep is None else np.ascontiguousarray(keep).astype(np.uint8)
        if kp.shape != (len(seg) - 1,):
            raise ValueError("orders_set: keep must be [n_seg]")
        self._od_key = None
        if self._dt_per_order:   # (new orders drop a per-order filter)
            self._dt_key = None
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.prom_orders_set(self.h, len(pm), len(seg) - 1, seg.ctypes.data_as(ip),
                                             pm.ctypes.data_as(ip), kp.ctypes.data_as(C.POINTER(C.c_uint8))),
                    "prom_orders_set")
        self._od_key = key
        self._od_n_seg = len(seg) - 1

    @property
    def orders_key(self):
        """The ``key`` of the orders resident on the context (None: none, or set without a key)."""
        return self._od_key

    def _orders_outputs(self, moments: bool, records: bool, totals: bool, model: bool):
        (mom, nu, mod), ptr = self._expose_outputs(moments, model)
        n_exp, n_trial, _ = self._ex_shape or (0, 0, 0)
        rm = np.zeros((n_exp, n_trial, self._od_n_seg, 7)) if records else None
        rn = np.zeros((n_exp, n_trial, self._od_n_seg), dtype=np.int64) if records else None
        tot = np.zeros((n_exp, n_trial, 4)) if totals else None
        ptr = (ptr[0], ptr[1], _d(rm) if records else None, rn.ctypes.data_as(C.POINTER(C.c_int64)) if records else None,
               _d(tot) if totals else None, ptr[2])
        return (mom, nu, rm, rn, tot, mod), ptr

    def transit_expose_orders(self, highpass: bool = False, detrend: bool = False, moments: bool = True,
                              records: bool = True, totals: bool = True, model: bool = False):
        """prom_transit_expose_orders over the last run's R: (moments [n_exp][n_trial][7], n_used [n_exp][n_trial],
        order moments [n_exp][n_trial][n_seg][7], order n_used [n_exp][n_trial][n_seg], totals [n_exp][n_trial][4] =
        (loglike, chi2, chi2_scaled, n_used) over the entering orders, final model [n_exp][n_trial][n_pix]), None for
        what was not asked.  ``highpass`` / ``detrend``: the resident high-pass, then the resident filter, run first."""
        out, ptr = self._orders_outputs(moments, records, totals, model)
        self._check(self.lib.prom_transit_expose_orders(self.h, int(highpass), int(detrend), *ptr),
                    "prom_transit_expose_orders")
        return out

    def spectrum_expose_orders(self, wav, R, highpass: bool = False, detrend: bool = False, moments: bool = True,
                               records: bool = True, totals: bool = True, model: bool = False):
        """prom_spectrum_expose_orders of R[n_orb][n_wav] on the ascending grid wav: transit_expose_orders' tuple."""
        wav, R = _spectrum(wav, R, "spectrum_expose_orders")
        out, ptr = self._orders_outputs(moments, records, totals, model)
        self._check(self.lib.prom_spectrum_expose_orders(self.h, R.shape[0], len(wav), _d(wav), _d(R), int(highpass),
                                                         int(detrend), *ptr), "prom_spectrum_expose_orders")
        return out

    def orders_kernel_ms(self, n_runs: int = 20):
        """prom_orders_kernel_ms: mean device durations [ms] of (k_order_moments, k_order_totals) over the whole table
        for the last per-order call."""
        ms = (C.c_double * 2)()
        self._check(self.lib.prom_orders_kernel_ms(self.h, int(n_runs), ms), "prom_orders_kernel_ms")
        return float(ms[0]), float(ms[1])

    # ---- broadened spectra (prom_hip.h "broadened spectra on the device") -----------------------
    def broaden_set(self, K, b0: float, s: float, key=None) -> None:
        """prom_broaden_set: the velocity kernel K [n_k] (2 <= n_k <= 1025, >= 0) with nodes at the Doppler offsets
        b0 + i / s.  ``key``: any value the caller keeps in ``broaden_key`` to skip a later upload of the same
        kernel."""
        K = _f64(K)
        if K.ndim != 1:
            raise ValueError("broaden_set: K must be a 1-D array")
        self._br_key = None
        self._check(self.lib.prom_broaden_set(self.h, len(K), float(b0), float(s), _d(K)), "prom_broaden_set")
        self._br_key = key

    def broaden_drop(self) -> None:
        """prom_broaden_set with n_k = 0: no kernel is resident any more."""
        self._br_key = None
        self._check(self.lib.prom_broaden_set(self.h, 0, 0.0, 1.0, None), "prom_broaden_set")

    @property
    def broaden_key(self):
        """The ``key`` of the kernel resident on the context (None: none, or set without a key)."""
        return self._br_key

    def spectrum_broaden(self, wav, R) -> np.ndarray:
        """prom_spectrum_broaden of R[n_orb][n_wav] on the ascending, positive grid wav: R_b[n_orb][n_wav]."""
        wav, R = _spectrum(wav, R, "spectrum_broaden")
        out = np.empty(R.shape)
        self._check(self.lib.prom_spectrum_broaden(self.h, R.shape[0], len(wav), _d(wav), _d(R), _d(out)),
                    "prom_spectrum_broaden")
        return out

    def transit_broaden(self) -> None:
        """prom_transit_broaden: R_b of the last run's R; the transit observe, vmap and expose calls read it until
        the next run."""
        self._check(self.lib.prom_transit_broaden(self.h), "prom_transit_broaden")

    def transit_broadened(self) -> np.ndarray:
        """prom_transit_broadened: the current R_b, [n_orb, n_wav]."""
        out = np.empty(getattr(self, "_shape", (1, 1)))   # (no problem set yet: the library refuses)
        self._check(self.lib.prom_transit_broadened(self.h, _d(out)), "prom_transit_broadened")
        return out

    def broaden_kernel_ms(self, n_runs: int = 20) -> float:
        """prom_broaden_kernel_ms: mean device duration [ms] of k_broaden for the last broaden call's launch."""
        ms = C.c_double(0.0)
        self._check(self.lib.prom_broaden_kernel_ms(self.h, int(n_runs), C.byref(ms)), "prom_broaden_kernel_ms")
        return float(ms.value)

    # ---- injection and SYSREM (prom_hip.h "injection and SYSREM on the device") -----------------
    def sysrem_set(self, raw, key=None) -> None:
        """prom_sysrem_set: the raw exposures raw [n_exp][n_pix] of the resident exposure table, in the device's pixel
        order (any value; NaN marks a bad pixel).  ``key``: any value the caller keeps in ``sysrem_key`` to skip a
        later upload of the same data."""
        raw = _f64(raw)
        if raw.ndim != 2:
            raise ValueError("sysrem_set: raw must be [n_exp][n_pix]")
        self._sy_key = None
        self._check(self.lib.prom_sysrem_set(self.h, raw.shape[0], raw.shape[1], _d(raw)), "prom_sysrem_set")
        self._sy_key = key

    @property
    def sysrem_key(self):
        """The ``key`` of the raw exposures resident on the context (None: none, or set without a key)."""
        return self._sy_key

    def _sysrem_outputs(self, n_comp: int, ones: bool, injected: bool, orders: bool = False):
        n_exp, _, n_pix = self._ex_shape or (0, 0, 0)
        U = np.zeros((n_exp, max(int(n_comp) + int(bool(ones)), 0)))
        if orders:   # (per order: a basis per resident order)
            U = np.zeros((self._od_n_seg,) + U.shape)
        cleaned = np.full((n_exp, n_pix), np.nan)
        inj = np.full((n_exp, n_pix), np.nan) if injected else None
        return (U, cleaned, inj), (_d(U), _d(cleaned), _d(inj) if injected else None)

    def sysrem_clean(self, n_comp: int, n_iter: int = 30, ones: bool = False, highpass: bool = False,
                     injected: bool = False):
        """prom_sysrem_clean: SYSREM of the resident raw exposures, after the resident high-pass with ``highpass``:
        (U [n_exp][n_comp + ones], cleaned [n_exp][n_pix], injected [n_exp][n_pix] or None), device pixel order."""
        out, ptr = self._sysrem_outputs(n_comp, ones, injected)
        self._check(self.lib.prom_sysrem_clean(self.h, int(bool(highpass)), int(n_comp), int(n_iter), int(bool(ones)),
                                               *ptr), "prom_sysrem_clean")
        return out

    def transit_inject(self, trial: int, scale: float, n_comp: int, n_iter: int = 30, ones: bool = False,
                       highpass: bool = False, injected: bool = False):
        """prom_transit_inject: the same after multiplying trial ``trial`` of the last run's model into the raw
        exposures at ``scale``."""
        out, ptr = self._sysrem_outputs(n_comp, ones, injected)
        self._check(self.lib.prom_transit_inject(self.h, int(trial), float(scale), int(bool(highpass)), int(n_comp),
                                                 int(n_iter), int(bool(ones)), *ptr), "prom_transit_inject")
        return out

    def spectrum_inject(self, wav, R, trial: int, scale: float, n_comp: int, n_iter: int = 30, ones: bool = False,
                        highpass: bool = False, injected: bool = False):
        """prom_spectrum_inject: the same for R[n_orb][n_wav] on the ascending grid wav."""
        wav, R = _spectrum(wav, R, "spectrum_inject")
        out, ptr = self._sysrem_outputs(n_comp, ones, injected)
        self._check(self.lib.prom_spectrum_inject(self.h, R.shape[0], len(wav), _d(wav), _d(R), int(trial), float(scale),
                                                  int(bool(highpass)), int(n_comp), int(n_iter), int(bool(ones)), *ptr),
                    "prom_spectrum_inject")
        return out

    # ---- SYSREM per order (prom_hip.h "SYSREM per order on the device") ---------------------------
    def sysrem_clean_orders(self, n_comp: int, n_iter: int = 30, ones: bool = False, highpass: bool = False,
                            injected: bool = False):
        """prom_sysrem_clean_orders: sysrem_clean with every resident order (orders_set) cleaned on its own, in the
        launches of one call: (U [n_seg][n_exp][n_comp + ones], cleaned, injected or None)."""
        out, ptr = self._sysrem_outputs(n_comp, ones, injected, orders=True)
        self._check(self.lib.prom_sysrem_clean_orders(self.h, int(bool(highpass)), int(n_comp), int(n_iter),
                                                      int(bool(ones)), *ptr), "prom_sysrem_clean_orders")
        return out

    def transit_inject_orders(self, trial: int, scale: float, n_comp: int, n_iter: int = 30, ones: bool = False,
                              highpass: bool = False, injected: bool = False):
        """prom_transit_inject_orders: transit_inject with every resident order cleaned on its own."""
        out, ptr = self._sysrem_outputs(n_comp, ones, injected, orders=True)
        self._check(self.lib.prom_transit_inject_orders(self.h, int(trial), float(scale), int(bool(highpass)),
                                                        int(n_comp), int(n_iter), int(bool(ones)), *ptr),
                    "prom_transit_inject_orders")
        return out

    def spectrum_inject_orders(self, wav, R, trial: int, scale: float, n_comp: int, n_iter: int = 30,
                               ones: bool = False, highpass: bool = False, injected: bool = False):
        """prom_spectrum_inject_orders: the same for R[n_orb][n_wav] on the ascending grid wav."""
        wav, R = _spectrum(wav, R, "spectrum_inject_orders")
        out, ptr = self._sysrem_outputs(n_comp, ones, injected, orders=True)
        self._check(self.lib.prom_spectrum_inject_orders(self.h, R.shape[0], len(wav), _d(wav), _d(R), int(trial),
                                                         float(scale), int(bool(highpass)), int(n_comp), int(n_iter),
                                                         int(bool(ones)), *ptr), "prom_spectrum_inject_orders")
        return out

    def sysrem_kernel_ms(self, n_runs: int = 5):
        """prom_sysrem_kernel_ms: mean device durations [ms] of (the SYSREM loop, the injection, k_highpass) for the
        last clean or inject call; NaN for a stage that call did not have."""
        ms = (C.c_double * 3)(0.0, 0.0, 0.0)
        self._check(self.lib.prom_sysrem_kernel_ms(self.h, int(n_runs), ms), "prom_sysrem_kernel_ms")
        return float(ms[0]), float(ms[1]), float(ms[2])

    # ---- the filter's weights and the recovery (prom_hip.h "the filter's weights on the device") ----
    def filter_weights(self, U, ivar) -> np.ndarray:
        """prom_filter_weights: W [n_comp][n_exp][n_pix] of U [n_exp][n_comp] (finite, 1 <= n_comp <= 16) and ivar
        [n_exp][n_pix] (any value), by the device's definition.  No table is needed."""
        U, ivar = _f64(U), _f64(ivar)
        if U.ndim != 2 or ivar.ndim != 2 or ivar.shape[0] != U.shape[0]:
            raise ValueError("filter_weights: U must be [n_exp][n_comp] and ivar [n_exp][n_pix]")
        n_exp, n_comp = U.shape
        W = np.zeros((n_comp, n_exp, ivar.shape[1]))
        self._check(self.lib.prom_filter_weights(self.h, n_exp, n_comp, ivar.shape[1], _d(U), _d(ivar), _d(W)),
                    "prom_filter_weights")
        return W

    def detrend_build(self, U, key=None, weights: bool = False):
        """prom_detrend_build: the filter of the resident exposure table from U [n_exp][n_comp] alone; W is formed on
        the device over the table's ivar and returned ([n_comp][n_exp][n_pix], device pixel order) with ``weights``.
        ``key``: as detrend_set's."""
        U = _f64(U)
        if U.ndim != 2:
            raise ValueError("detrend_build: U must be [n_exp][n_comp]")
        n_exp, n_comp = U.shape
        n_pix = (self._ex_shape or (0, 0, 0))[2]
        W = np.zeros((n_comp, n_exp, n_pix)) if weights else None
        self._dt_key = None
        self._check(self.lib.prom_detrend_build(self.h, n_exp, n_comp, _d(U), _d(W) if weights else None),
                    "prom_detrend_build")
        self._dt_key = key
        self._dt_per_order = False
        return W

    # ---- the filter per order (prom_hip.h "SYSREM per order on the device") -----------------------
    def filter_weights_orders(self, U, ivar, seg_of) -> np.ndarray:
        """prom_filter_weights_orders: W [n_comp][n_exp][n_pix] of U [n_seg][n_exp][n_comp], ivar [n_exp][n_pix] and
        seg_of [n_pix] (int32, the order of every pixel): pixel p is given the basis U[seg_of[p]]."""
        U, ivar = _f64(U), _f64(ivar)
        sg = np.ascontiguousarray(seg_of, dtype=np.int32)
        if U.ndim != 3 or ivar.ndim != 2 or ivar.shape[0] != U.shape[1] or sg.shape != (ivar.shape[1],):
            raise ValueError("filter_weights_orders: U must be [n_seg][n_exp][n_comp], ivar [n_exp][n_pix] and seg_of "
                             "[n_pix]")
        n_seg, n_exp, n_comp = U.shape
        W = np.zeros((n_comp, n_exp, ivar.shape[1]))
        self._check(self.lib.prom_filter_weights_orders(self.h, n_exp, n_comp, ivar.shape[1], n_seg,
                                                        sg.ctypes.data_as(_ip), _d(U), _d(ivar), _d(W)),
                    "prom_filter_weights_orders")
        return W

    def detrend_set_orders(self, U, W, key=None) -> None:
        """prom_detrend_set_orders: the per-order filter of the resident exposure table: U [n_seg][n_exp][n_comp], a
        basis per resident order (orders_set), and W [n_comp][n_exp][n_pix] in the device's pixel order.  Every
        detrended call afterwards filters pixel p with the basis of its own order; detrend_set / detrend_build put the
        single basis back, orders_set drops the filter.  ``key``: as detrend_set's."""
        U, W = _f64(U), _f64(W)
        if U.ndim != 3 or W.ndim != 3 or W.shape[:2] != (U.shape[2], U.shape[1]):
            raise ValueError("detrend_set_orders: U must be [n_seg][n_exp][n_comp] and W [n_comp][n_exp][n_pix]")
        self._dt_key = None
        n_seg, n_exp, n_comp = U.shape
        self._check(self.lib.prom_detrend_set_orders(self.h, n_exp, n_comp, n_seg, _d(U), _d(W)),
                    "prom_detrend_set_orders")
        self._dt_key = key
        self._dt_per_order = True

    def detrend_build_orders(self, U, key=None, weights: bool = False):
        """prom_detrend_build_orders: the per-order filter from U [n_seg][n_exp][n_comp] alone; W is formed on the
        device over the table's ivar, every pixel with its own order's basis, and returned with ``weights``."""
        U = _f64(U)
        if U.ndim != 3:
            raise ValueError("detrend_build_orders: U must be [n_seg][n_exp][n_comp]")
        n_seg, n_exp, n_comp = U.shape
        n_pix = (self._ex_shape or (0, 0, 0))[2]
        W = np.zeros((n_comp, n_exp, n_pix)) if weights else None
        self._dt_key = None
        self._check(self.lib.prom_detrend_build_orders(self.h, n_exp, n_comp, n_seg, _d(U),
                                                       _d(W) if weights else None), "prom_detrend_build_orders")
        self._dt_key = key
        self._dt_per_order = True
        return W

    def filter_kernel_ms(self, n_runs: int = 20) -> float:
        """prom_filter_kernel_ms: mean device duration [ms] of k_filter_weights for the last build or recover call."""
        ms = C.c_double(0.0)
        self._check(self.lib.prom_filter_kernel_ms(self.h, int(n_runs), C.byref(ms)), "prom_filter_kernel_ms")
        return float(ms.value)

    def _recover_outputs(self, n_comp: int, ones: bool, orders: bool, moments: bool, records: bool, totals: bool,
                         model: bool):
        n_exp = (self._ex_shape or (0, 0, 0))[0]
        U = np.zeros((n_exp, max(int(n_comp) + int(bool(ones)), 0)))
        if orders:
            out, ptr = self._orders_outputs(moments, records, totals, model)
        else:
            (mom, nu, mod), p = self._expose_outputs(moments, model)
            out, ptr = (mom, nu, None, None, None, mod), (p[0], p[1], None, None, None, p[2])
        return out + (U,), ptr[:5] + (_d(U), ptr[5])

    def transit_recover(self, trial: int, scale: float, n_comp: int, n_iter: int = 30, ones: bool = False,
                        highpass: bool = False, orders: bool = False, moments: bool = True, records: bool = True,
                        totals: bool = True, model: bool = False):
        """prom_transit_recover: trial ``trial`` of the last run's model injected at ``scale``, cleaned, and the whole
        table's filtered model met with the cleaned data, all on the device: (moments, n_used, order moments, order
        n_used, totals, final model, U [n_exp][n_comp + ones]); the per-order entries are None without ``orders``."""
        out, ptr = self._recover_outputs(n_comp, ones, orders, moments, records, totals, model)
        self._check(self.lib.prom_transit_recover(self.h, int(trial), float(scale), int(bool(highpass)), int(n_comp),
                                                  int(n_iter), int(bool(ones)), int(bool(orders)), *ptr),
                    "prom_transit_recover")
        return out

    def spectrum_recover(self, wav, R, trial: int, scale: float, n_comp: int, n_iter: int = 30, ones: bool = False,
                         highpass: bool = False, orders: bool = False, moments: bool = True, records: bool = True,
                         totals: bool = True, model: bool = False):
        """prom_spectrum_recover: the same for R[n_orb][n_wav] on the ascending grid wav."""
        wav, R = _spectrum(wav, R, "spectrum_recover")
        out, ptr = self._recover_outputs(n_comp, ones, orders, moments, records, totals, model)
        self._check(self.lib.prom_spectrum_recover(self.h, R.shape[0], len(wav), _d(wav), _d(R), int(trial),
                                                   float(scale), int(bool(highpass)), int(n_comp), int(n_iter),
                                                   int(bool(ones)), int(bool(orders)), *ptr), "prom_spectrum_recover")
        return out

    # ---- injection grids (prom_hip.h "injection grids on the device") ---------------------------
    @staticmethod
    def _grid_list(trials, scales, who: str):
        """The list of a grid call as (n_inj, int32 trials, float64 scales), one entry per injection."""
        t = np.ascontiguousarray(trials, dtype=np.int32)
        s = np.ascontiguousarray(scales, dtype=np.float64)
        if t.ndim != 1 or s.shape != t.shape:
            raise ValueError("%s: trials and scales must be two lists of one length" % who)
        return len(t), t, s

    def _inject_grid_outputs(self, n_inj: int, n_comp: int, ones: bool, data: bool, injected: bool,
                             orders: bool = False):
        n_exp, _, n_pix = self._ex_shape or (0, 0, 0)
        U = np.zeros((n_inj,) + ((self._od_n_seg,) if orders else ()) + (n_exp, max(int(n_comp) + int(bool(ones)), 0)))
        cleaned = np.full((n_inj, n_exp, n_pix), np.nan) if data else None
        inj = np.full((n_inj, n_exp, n_pix), np.nan) if injected else None
        return (U, cleaned, inj), (_d(U), _d(cleaned) if data else None, _d(inj) if injected else None)

    def transit_inject_grid(self, trials, scales, n_comp: int, n_iter: int = 30, ones: bool = False,
                            highpass: bool = False, data: bool = True, injected: bool = False):
        """prom_transit_inject_grid: every (trials[b], scales[b]) injected into the raw exposures from the last run's
        model and cleaned, in one call: (U [n_inj][n_exp][n_comp + ones], cleaned [n_inj][n_exp][n_pix] or None
        without ``data``, injected likewise or None), entry b what transit_inject gives for that point."""
        n_inj, t, s = self._grid_list(trials, scales, "transit_inject_grid")
        out, ptr = self._inject_grid_outputs(n_inj, n_comp, ones, data, injected)
        self._check(self.lib.prom_transit_inject_grid(self.h, n_inj, t.ctypes.data_as(_ip), _d(s), int(bool(highpass)),
                                                      int(n_comp), int(n_iter), int(bool(ones)), *ptr),
                    "prom_transit_inject_grid")
        return out

    def spectrum_inject_grid(self, wav, R, trials, scales, n_comp: int, n_iter: int = 30, ones: bool = False,
                             highpass: bool = False, data: bool = True, injected: bool = False):
        """prom_spectrum_inject_grid: the same for R[n_orb][n_wav] on the ascending grid wav."""
        wav, R = _spectrum(wav, R, "spectrum_inject_grid")
        n_inj, t, s = self._grid_list(trials, scales, "spectrum_inject_grid")
        out, ptr = self._inject_grid_outputs(n_inj, n_comp, ones, data, injected)
        self._check(self.lib.prom_spectrum_inject_grid(self.h, R.shape[0], len(wav), _d(wav), _d(R), n_inj,
                                                       t.ctypes.data_as(_ip), _d(s), int(bool(highpass)), int(n_comp),
                                                       int(n_iter), int(bool(ones)), *ptr),
                    "prom_spectrum_inject_grid")
        return out

    def transit_inject_grid_orders(self, trials, scales, n_comp: int, n_iter: int = 30, ones: bool = False,
                                   highpass: bool = False, data: bool = True, injected: bool = False):
        """prom_transit_inject_grid_orders: transit_inject_grid with every resident order cleaned on its own: U is
        [n_inj][n_seg][n_exp][n_comp + ones], entry b what transit_inject_orders gives for that point."""
        n_inj, t, s = self._grid_list(trials, scales, "transit_inject_grid_orders")
        out, ptr = self._inject_grid_outputs(n_inj, n_comp, ones, data, injected, orders=True)
        self._check(self.lib.prom_transit_inject_grid_orders(self.h, n_inj, t.ctypes.data_as(_ip), _d(s),
                                                             int(bool(highpass)), int(n_comp), int(n_iter),
                                                             int(bool(ones)), *ptr), "prom_transit_inject_grid_orders")
        return out

    def spectrum_inject_grid_orders(self, wav, R, trials, scales, n_comp: int, n_iter: int = 30, ones: bool = False,
                                    highpass: bool = False, data: bool = True, injected: bool = False):
        """prom_spectrum_inject_grid_orders: the same for R[n_orb][n_wav] on the ascending grid wav."""
        wav, R = _spectrum(wav, R, "spectrum_inject_grid_orders")
        n_inj, t, s = self._grid_list(trials, scales, "spectrum_inject_grid_orders")
        out, ptr = self._inject_grid_outputs(n_inj, n_comp, ones, data, injected, orders=True)
        self._check(self.lib.prom_spectrum_inject_grid_orders(self.h, R.shape[0], len(wav), _d(wav), _d(R), n_inj,
                                                              t.ctypes.data_as(_ip), _d(s), int(bool(highpass)),
                                                              int(n_comp), int(n_iter), int(bool(ones)), *ptr),
                    "prom_spectrum_inject_grid_orders")
        return out

    def _recover_grid_outputs(self, n_inj: int, n_comp: int, ones: bool, orders: bool, moments: bool, totals: bool):
        n_exp, n_trial, _ = self._ex_shape or (0, 0, 0)
        U = np.zeros((n_inj, n_exp, max(int(n_comp) + int(bool(ones)), 0)))
        mom = np.zeros((n_inj, n_exp, n_trial, 7)) if moments else None
        nu = np.zeros((n_inj, n_exp, n_trial), dtype=np.int64) if moments else None
        tot = np.zeros((n_inj, n_exp, n_trial, 4)) if orders and totals else None
        return (mom, nu, tot, U), (_d(mom) if moments else None,
                                   nu.ctypes.data_as(C.POINTER(C.c_int64)) if moments else None,
                                   _d(tot) if tot is not None else None, _d(U))

    def transit_recover_grid(self, trials, scales, n_comp: int, n_iter: int = 30, ones: bool = False,
                             highpass: bool = False, orders: bool = False, moments: bool = True, totals: bool = True):
        """prom_transit_recover_grid: every (trials[b], scales[b]) injected, cleaned and recovered in one call:
        (moments [n_inj][n_exp][n_trial][7], n_used [n_inj][n_exp][n_trial], totals [n_inj][n_exp][n_trial][4] or None
        without ``orders``, U [n_inj][n_exp][n_comp + ones]), entry b what transit_recover gives for that point."""
        n_inj, t, s = self._grid_list(trials, scales, "transit_recover_grid")
        out, ptr = self._recover_grid_outputs(n_inj, n_comp, ones, orders, moments, totals)
        self._check(self.lib.prom_transit_recover_grid(self.h, n_inj, t.ctypes.data_as(_ip), _d(s), int(bool(highpass)),
                                                       int(n_comp), int(n_iter), int(bool(ones)), int(bool(orders)),
                                                       *ptr), "prom_transit_recover_grid")
        return out

    def spectrum_recover_grid(self, wav, R, trials, scales, n_comp: int, n_iter: int = 30, ones: bool = False,
                              highpass: bool = False, orders: bool = False, moments: bool = True, totals: bool = True):
        """prom_spectrum_recover_grid: the same for R[n_orb][n_wav] on the ascending grid wav."""
        wav, R = _spectrum(wav, R, "spectrum_recover_grid")
        n_inj, t, s = self._grid_list(trials, scales, "spectrum_recover_grid")
        out, ptr = self._recover_grid_outputs(n_inj, n_comp, ones, orders, moments, totals)
        self._check(self.lib.prom_spectrum_recover_grid(self.h, R.shape[0], len(wav), _d(wav), _d(R), n_inj,
                                                        t.ctypes.data_as(_ip), _d(s), int(bool(highpass)), int(n_comp),
                                                        int(n_iter), int(bool(ones)), int(bool(orders)), *ptr),
                    "prom_spectrum_recover_grid")
        return out

    # ---- stellar disk -----------------------------------------------------------------------
    def star_disk_flux(self, table_id: int, shift, clv, rho, dphi: float, drho: float, wavelength) -> np.ndarray:
        """prom_star_disk_flux: sum over disk cells (in order) of 10^interp(lambda / shift) clv dphi drho rho."""
        sh, cl, rh, w = _f64(shift), _f64(clv), _f64(rho), _f64(wavelength)
        if not (len(sh) == len(cl) == len(rh)):
            raise ValueError("shift, clv and rho need one value per disk cell")
        out = np.empty(w.shape)
        self._check(self.lib.prom_star_disk_flux(self.h, int(table_id), len(sh), _d(sh), _d(cl), _d(rh), float(dphi),
                                                 float(drho), w.size, _d(w), _d(out)), "prom_star_disk_flux")
        return out


class TransitInputs:
    """Owns the numpy arrays behind one prom_transit_problem (kept alive while in use)."""

    def __init__(self, *, wavelength, chord_y, chord_z, chord_fout, n_orb, x, delta_x, planet_y, planet_R,
                 moon_y, moon_R, scenarios, cull_tau=0.0, options=0, k_B=0.0, star=None):
        keep = []

        def arr(a):
            a = _f64(a)
            keep.append(a)
            return a

        s = TransitProblem()
        w = arr(wavelength)
        s.n_wav, s.wavelength = len(w), _d(w)
        cy, cz, cf = arr(chord_y), arr(chord_z), arr(chord_fout)
        s.n_pr, s.chord_y, s.chord_z, s.chord_fout = len(cy), _d(cy), _d(cz), _d(cf)
        s.n_orb = int(n_orb)
        xx = arr(x)
        s.n_x, s.x, s.delta_x = len(xx), _d(xx), float(delta_x)
        py = arr(planet_y)
        s.planet_y, s.planet_R = _d(py), float(planet_R)
        s.n_moons = len(moon_R)
        my, mr = arr(np.reshape(moon_y, (-1,)) if len(moon_R) else np.zeros(1)), arr(moon_R if len(moon_R) else np.zeros(1))
        s.moon_y, s.moon_R = _d(my), _d(mr)
        scs = (Scenario * len(scenarios))()
        n_atoms = 0
        for i, sc in enumerate(scenarios):
            d = scs[i]
            d.density.kind = int(sc["kind"])
            for j, v in enumerate(sc.get("params", ())):
                d.density.p[j] = float(v)
            if sc.get("body_x") is not None:
                d.body_x, d.body_y = _d(arr(sc["body_x"])), _d(arr(sc["body_y"]))
            d.shift = _d(arr(sc["shift"]))
            if sc.get("n_tabulated") is not None:
                d.n_tabulated = _d(arr(sc["n_tabulated"]))
            d.T = float(sc.get("T", 0.0))
            cons = sc["constituents"]
            ca = (Constituent * max(1, len(cons)))()
            for k, c in enumerate(cons):
                ca[k].table_id = int(c["table_id"])
                ca[k].is_molecule = int(bool(c.get("is_molecule", False)))
                ca[k].chi = float(c["chi"])
                n_atoms += 0 if c.get("is_molecule", False) else 1
            keep.append(ca)
            d.n_constituents = len(cons)
            d.constituents = ca
        keep.append(scs)
        s.n_scenarios = len(scenarios)
        s.scenarios = scs
        s.cull_tau = float(cull_tau)
        s.options = int(options)
        s.k_B = float(k_B)
        if star is not None:
            # {"table_id", "rho", "clv", "shift"}: stellar spectrum path (prom_hip.h has_star)
            s.has_star, s.star_table = 1, int(star["table_id"])
            s.chord_rho, s.chord_clv = _d(arr(star["rho"])), _d(arr(star["clv"]))
            s.chord_star_shift = _d(arr(star["shift"]))
        self.struct = s
        self.keepalive = keep
        self.n_atoms = n_atoms
        self.n_molecules = sum(1 for sc in scenarios for c in sc["constituents"] if c.get("is_molecule", False))


_default_device = int(os.environ.get("PROMETHEUS_DEVICE", "0"))


def set_default_device(device: int) -> None:
    """GPU used by calls that do not name one (table builds, plugin methods)."""
    global _default_device
    _default_device = int(device)


def default_device() -> int:
    return _default_device


_ctx_lock = threading.Lock()
_contexts: Dict[int, Device] = {}


def get_device(device: int = 0) -> Device:
    """Process-wide context of one GPU.  Serialise use with ``dev.lock`` (one host thread per
    device at a time; different devices run concurrently, ctypes drops the GIL)."""
    key = int(device)
    with _ctx_lock:
        d = _contexts.get(key)
        if d is None:
            d = Device(device)
            d.lock = threading.RLock()
            _contexts[key] = d
        return d
