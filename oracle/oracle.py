"""ctypes wrapper for the CPU oracle (oracle/liboracle.so) — TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import
this module, as the checker / CPU baseline. The product path never does.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liboracle.so")

LEX, RB = 0, 1
CAVITY, CHANNEL, BACKSTEP, RAYLEIGH_BENARD = range(4)  # enum ORC_CAVITY .. ORC_RBC
F_P, F_SRC, F_RES, F_US, F_VS, F_U, F_V, F_UC, F_VC, F_T, F_T2 = range(11)
FIELD_IDS = {"p": F_P, "src": F_SRC, "res": F_RES, "us": F_US, "vs": F_VS, "u": F_U, "v": F_V, "uc": F_UC,
             "vc": F_VC, "t": F_T}


class OrcParams(ctypes.Structure):
    _fields_ = [
        ("case_id", ctypes.c_int), ("nx", ctypes.c_int), ("ny", ctypes.c_int),
        ("dx", ctypes.c_double), ("dy", ctypes.c_double), ("nu", ctypes.c_double), ("rho", ctypes.c_double),
        ("u_ref", ctypes.c_double), ("dt", ctypes.c_double), ("omega", ctypes.c_double),
        ("tol_factor", ctypes.c_double), ("abs_tol", ctypes.c_double), ("max_iters", ctypes.c_int),
        ("step_i", ctypes.c_int), ("inlet_jmax", ctypes.c_int),
        ("kappa", ctypes.c_double), ("buoyancy", ctypes.c_double), ("t_hot", ctypes.c_double),
        ("t_cold", ctypes.c_double), ("t_ref", ctypes.c_double), ("t_perturb", ctypes.c_double),
        ("length", ctypes.c_double),
    ]


_lib = None


def build() -> None:
    subprocess.check_call(["make", "-s", "-C", HERE])


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        L = ctypes.CDLL(LIB_PATH)
        L.orc_create.restype = ctypes.c_void_p
        L.orc_create.argtypes = [ctypes.POINTER(OrcParams)]
        L.orc_destroy.argtypes = [ctypes.c_void_p]
        L.orc_field.restype = ctypes.POINTER(ctypes.c_double)
        L.orc_field.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.orc_mask.restype = ctypes.POINTER(ctypes.c_ubyte)
        L.orc_mask.argtypes = [ctypes.c_void_p]
        L.orc_fluid_count.argtypes = [ctypes.c_void_p]
        for name in ("orc_tentative", "orc_correct", "orc_centers"):
            getattr(L, name).argtypes = [ctypes.c_void_p]
        L.orc_velocity_bc.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.orc_source.restype = ctypes.c_double
        L.orc_source.argtypes = [ctypes.c_void_p]
        L.orc_source_raw.restype = ctypes.c_double
        L.orc_source_raw.argtypes = [ctypes.c_void_p]
        L.orc_subtract_mean.argtypes = [ctypes.c_void_p, ctypes.c_double]
        ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
        L.orc_poisson.argtypes = [ctypes.c_void_p, ctypes.c_int, ip, dp]
        L.orc_poisson_every.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ip, dp]
        L.orc_poisson_fixed.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, dp]
        L.orc_step.argtypes = [ctypes.c_void_p, ctypes.c_int, ip, dp]
        L.orc_stats.argtypes = [ctypes.c_void_p, dp, dp]
        L.orc_temperature_bc.argtypes = [ctypes.c_void_p]
        L.orc_thermal.argtypes = [ctypes.c_void_p]
        L.orc_nusselt.restype = ctypes.c_double
        L.orc_nusselt.argtypes = [ctypes.c_void_p]
        L.orc_omega_square.restype = ctypes.c_double
        L.orc_omega_square.argtypes = [ctypes.c_int]
        L.orc_omega_2d.restype = ctypes.c_double
        L.orc_omega_2d.argtypes = [ctypes.c_int, ctypes.c_int]
        _lib = L
    return _lib


def params_from_case(p) -> OrcParams:
    """Build oracle parameters from a cfd_amd.params.CaseParams."""
    return OrcParams(p.case_id, p.nx, p.ny, p.dx, p.dy, p.nu, p.rho, p.u_ref, p.dt, p.omega, p.tol_factor,
                     p.abs_tol, p.max_iters, p.step_i, p.inlet_jmax, getattr(p, "kappa", 0.0),
                     getattr(p, "buoyancy", 0.0), getattr(p, "t_hot", 1.0), getattr(p, "t_cold", 0.0),
                     getattr(p, "t_ref", 0.0), getattr(p, "t_perturb", 0.0), p.length)


class Oracle:
    """Reference-algorithm CPU solver; fields are (ny+2, nx+2) numpy views."""

    def __init__(self, case_params, ordering: int = LEX):
        self.cp = case_params
        self.ordering = ordering
        self._p = params_from_case(case_params)
        self.h = lib().orc_create(ctypes.byref(self._p))
        if not self.h:
            raise RuntimeError("orc_create failed")
        self.shape = (case_params.ny + 2, case_params.nx + 2)

    def __del__(self):
        if getattr(self, "h", None):
            lib().orc_destroy(self.h)
            self.h = None

    def field(self, name: str) -> np.ndarray:
        ptr = lib().orc_field(self.h, FIELD_IDS[name])
        return np.ctypeslib.as_array(ptr, shape=self.shape)

    def mask(self) -> np.ndarray:
        return np.ctypeslib.as_array(lib().orc_mask(self.h), shape=self.shape)

    def fluid_count(self) -> int:
        return lib().orc_fluid_count(self.h)

    # reference phases
    def velocity_bc(self, tentative: bool = False) -> None:
        lib().orc_velocity_bc(self.h, int(tentative))

    def tentative(self) -> None:
        lib().orc_tentative(self.h)

    def source(self, total=None) -> float:
        """total: None (the reference's sequential sum of the open cases' mean
        removal) or a callable raw_f -> total that restates another summation
        order (tests/rb_sums.py: the GPU's red-black tree sum). The cavity and
        Rayleigh-Benard remove no mean: total is not called."""
        if total is None or self.cp.case_id in (CAVITY, RAYLEIGH_BENARD):
            return lib().orc_source(self.h)
        m = lib().orc_source_raw(self.h)
        if m > 0:
            lib().orc_subtract_mean(self.h, float(total(self.field("src"))))
        return m

    def kinetic_energy(self, ke_total) -> float:
        """The average kinetic energy of orc_stats with its sum restated: ke_total is a
        callable (uc, vc) -> the sum of 0.5 * (uc*uc + vc*vc) over the fluid cells. Run
        after centers() (or stats())."""
        return float(ke_total(self.field("uc"), self.field("vc"))) / float(self.fluid_count())

    def poisson(self, ordering: int | None = None, check_every: int = 1) -> tuple[int, float]:
        """check_every > 1: the stop rule on multiples of check_every only (orc_poisson_every)."""
        it, res = ctypes.c_int(), ctypes.c_double()
        o = self.ordering if ordering is None else ordering
        if check_every == 1:
            lib().orc_poisson(self.h, o, ctypes.byref(it), ctypes.byref(res))
        else:
            lib().orc_poisson_every(self.h, o, check_every, ctypes.byref(it), ctypes.byref(res))
        return it.value, res.value

    def poisson_every(self, check_every: int, ordering: int | None = None) -> tuple[int, float]:
        it, res = ctypes.c_int(), ctypes.c_double()
        lib().orc_poisson_every(self.h, self.ordering if ordering is None else ordering, check_every,
                                ctypes.byref(it), ctypes.byref(res))
        return it.value, res.value

    def poisson_fixed(self, n: int, ordering: int | None = None) -> float:
        res = ctypes.c_double()
        lib().orc_poisson_fixed(self.h, self.ordering if ordering is None else ordering, n, ctypes.byref(res))
        return res.value

    def correct(self) -> None:
        lib().orc_correct(self.h)

    def centers(self) -> None:
        lib().orc_centers(self.h)

    def stats(self) -> tuple[float, float]:
        md, ke = ctypes.c_double(), ctypes.c_double()
        lib().orc_stats(self.h, ctypes.byref(md), ctypes.byref(ke))
        return md.value, ke.value

    # Rayleigh-Benard phases (case 3; parity unpinned: no reference solver)
    def temperature_bc(self) -> None:
        lib().orc_temperature_bc(self.h)

    def thermal(self) -> None:
        lib().orc_thermal(self.h)

    def nusselt(self) -> float:
        return lib().orc_nusselt(self.h)

    def step(self, check_every: int = 1, source_total=None) -> tuple[int, float]:
        """source_total: as source(total=...), for the step's mean removal."""
        if check_every > 1 or source_total is not None:
            return self.step_phases(check_every, source_total)
        it, res = ctypes.c_int(), ctypes.c_double()
        lib().orc_step(self.h, self.ordering, ctypes.byref(it), ctypes.byref(res))
        return it.value, res.value

    def step_phases(self, check_every: int = 1, source_total=None) -> tuple[int, float]:
        """orc_step composed from the phases, in its order for the case, with
        the solve's stop rule tested every check_every iterations and the open
        cases' mean removal given source_total (source(total=...))."""
        case = self.cp.case_id
        if case in (CAVITY, RAYLEIGH_BENARD):
            self.velocity_bc(False)
            if case == RAYLEIGH_BENARD:
                self.temperature_bc()
            self.tentative()
            if case == RAYLEIGH_BENARD:
                self.thermal()
            self.source()
            r = self.poisson_every(check_every)
            self.correct()
            return r
        self.tentative()
        self.velocity_bc(True)
        self.source(source_total)
        r = self.poisson_every(check_every)
        self.correct()
        self.velocity_bc(False)
        return r
