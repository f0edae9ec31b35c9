"""CPU-side checks of the streamed below-ground surface (include/mcf.h mcf_plan_create_streamed / mcf_plan_below_prepare):
declared, exported and bound with the right signatures, the ABI version that announces them, the Python Plan's keyword and
method, and the options / inputs structs the ABI keeps unchanged."""
import ctypes as C
import inspect
import re
from pathlib import Path

from microclimf_amd import _abi
from microclimf_amd.api import Plan

ROOT = Path(__file__).resolve().parent.parent


def _lib():
    import __graft_entry__ as g
    g.build_library()
    return _abi.load()


def test_streamed_entries_are_declared_exported_and_bound():
    hdr = (ROOT / "include" / "mcf.h").read_text()
    assert re.search(r"int mcf_plan_create_streamed\(const mcf_grid_inputs \*in, const mcf_options \*opt,\s*int32_t ring_days, "
                     r"int32_t ring_slots, mcf_plan \*\*plan\);", hdr)
    assert "int mcf_plan_below_prepare(mcf_plan *plan, const mcf_grid_inputs *in);" in hdr
    assert int(re.search(r"#define MCF_ABI_VERSION (\d+)", hdr).group(1)) >= 7
    lib = _lib()
    assert lib.mcf_abi_version() == _abi.ABI_VERSION >= 7
    assert lib.mcf_plan_create_streamed.argtypes == lib.mcf_plan_create.argtypes
    assert lib.mcf_plan_create_streamed.restype is C.c_int
    assert lib.mcf_plan_below_prepare.restype is C.c_int
    assert len(lib.mcf_plan_below_prepare.argtypes) == 2


def test_null_plan_is_refused_without_touching_a_device():
    lib = _lib()
    assert lib.mcf_plan_below_prepare(None, None) == 1          # MCF_ERR_ARG
    assert b"null plan" in lib.mcf_last_error()


def test_plan_keyword_and_method():
    sig = inspect.signature(Plan.__init__)
    assert sig.parameters["stream_below"].default is False
    assert sig.parameters["stream_below"].kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(getattr(Plan, "below_prepare", None))


def test_options_and_inputs_keep_their_size():
    # the streamed plan is new entry points only: the structs test_abi_cpu.py pins are the same
    assert C.sizeof(_abi.Options) == 6 * 8 + 4 + 10 * 4 + 3 * 4
    assert not any(n in ("stream_below", "below_stream") for n, _ in _abi.Options._fields_)
