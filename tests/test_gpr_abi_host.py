"""The C ABI of the exact GPR class: the shared library exports the entry points include/cglb_hip.h declares and the ctypes binding lists them."""
import ctypes

from cglb_amd import _lib

SYMBOLS = ("cglb_gpr_set_hypers", "cglb_gpr_objective_and_grad", "cglb_gpr_predict")


def test_library_exports_the_gpr_entry_points():
    lib = ctypes.CDLL(_lib.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name), name


def test_binding_declares_the_gpr_entry_points():
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()
    assert lib.cglb_gpr_objective_and_grad.argtypes is not None
