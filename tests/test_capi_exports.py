"""The C-ABI library loads without a GPU and exports every symbol include/hml.h declares."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(REPO, "include", "hml.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(hml_[a-z0-9_]+)\s*\(", text))
    names.discard("hml_record_cb")
    return sorted(names)


def test_library_exports_every_declared_symbol():
    from hammlet_amd import build, capi
    build.build_library()
    lib = ctypes.CDLL(build.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 40
    for s in syms:
        assert hasattr(lib, s), s
    # the Python mirror binds exactly the declared surface
    assert sorted(capi.SIGNATURES) == syms


def test_library_holds_the_sweep_of_every_number_of_states():
    """hammlet_amd/build.py links the C ABI (csrc/hml_capi.hip, the recordings' read-outs csrc/hml_readout.hip and the exact
    inference csrc/hml_infer.hip, once each) and, per number of states
    2 ... 16, the sweep behind its table of function pointers (csrc/hml_sweep.hip with -DHML_TU_K=k) - one table per K must be there, and the objects of the
    build must be the ones the layout names (a stale single-object build would define the C ABI twice or not at all)."""
    from hammlet_amd import build
    build.build_library()
    objs = [o for _, o, _ in build._objects()]
    assert "hml_capi.o" in objs and all("hml_sweep_k%d.o" % k in objs for k in range(2, 17))
    assert "hml_readout.o" in objs and "hml_infer.o" in objs
    lib = ctypes.CDLL(build.LIB_PATH)
    for k in range(2, 17):
        tab = (ctypes.c_void_p * 5).in_dll(lib, "hml_ktab_%d" % k)
        assert all(tab[i] for i in range(5)), k       # sweep, iterate_many, params, compat_draw, derive
    with pytest.raises(ValueError):
        ctypes.c_void_p.in_dll(lib, "hml_ktab_17")


def test_no_gpu_means_a_loud_failure_not_a_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import hammlet_amd
    with pytest.raises(hammlet_amd.HmlError):
        hammlet_amd.Chain()


def test_memory_diagnostics_answer_without_a_gpu():
    """hml_device_memory_live and hml_debug_fail_allocation need no device: with no context alive the owners hold nothing,
    and the hook reports the allocations made since it was set - none here."""
    import torch
    import hammlet_amd
    hammlet_amd.debug_fail_allocation(0)
    assert hammlet_amd.debug_fail_allocation(3) == 0    # armed: nothing was allocated in between
    assert hammlet_amd.debug_fail_allocation(0) == 0    # ... and off again
    live = hammlet_amd.device_memory_live()
    if not torch.cuda.is_available():
        assert live == (0, 0)
    assert (live[0] == 0) == (live[1] == 0)


def test_guard_mode_answers_without_a_gpu():
    """hml_debug_guard_allocations and hml_debug_check_guards need no device: arming rounds the guard, registers nothing and
    restarts the allocation count; a check with nothing registered is clean.  The self-test needs device memory: without a
    GPU it is an error with a message, not a crash."""
    import torch
    import hammlet_amd
    hammlet_amd.debug_guard_allocations(1, poison=True)
    try:
        assert hammlet_amd.debug_check_guards(reset=False) == {"damaged": 0}
        assert hammlet_amd.debug_fail_allocation(0) == 0    # nothing was allocated since the mode was armed
    finally:
        hammlet_amd.debug_guard_allocations(0)
    assert hammlet_amd.debug_check_guards() == {"damaged": 0}
    with pytest.raises(hammlet_amd.HmlError):
        hammlet_amd.debug_guard_allocations(1 << 40)
    if not torch.cuda.is_available():
        with pytest.raises(hammlet_amd.HmlError) as e:
            hammlet_amd.debug_guard_selftest()
        assert e.value.code == 2 and "no HIP device" in str(e.value)    # HML_ERR_HIP
        assert hammlet_amd.device_memory_live() == (0, 0)


def test_product_never_references_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may touch oracle/."""
    for root in ("hammlet_amd", "include"):
        for dp, _, fns in os.walk(os.path.join(REPO, root)):
            for fn in fns:
                if fn.endswith((".py", ".h", ".hpp", ".hip", ".cpp")):
                    txt = open(os.path.join(dp, fn)).read().lower()
                    assert "oracle" not in txt, os.path.join(dp, fn)
