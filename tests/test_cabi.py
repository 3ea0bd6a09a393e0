"""The C-ABI library builds, loads, and exports every symbol include/*.h declares.
No compute calls (CPU-only container)."""
import ctypes
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    import proben_amd
    return proben_amd._lib.LIB_PATH


def declared_symbols():
    syms = set()
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        txt = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        syms |= set(re.findall(r"\b(pe_[a-z0-9_]+)\s*\(", txt))
    return sorted(syms)


def test_header_declares_entry_points():
    syms = declared_symbols()
    assert "pe_proben_fuse_batch" in syms and "pe_last_error" in syms


def test_library_exports_every_declared_symbol(built_lib):
    L = ctypes.CDLL(built_lib)
    missing = [s for s in declared_symbols() if not hasattr(L, s)]
    assert not missing, f"declared in include/*.h but not exported: {missing}"


def test_python_binding_covers_header(built_lib):
    import proben_amd
    bound = set(proben_amd._lib.SIGNATURES) | {"pe_last_error"}
    assert set(declared_symbols()) <= bound, set(declared_symbols()) - bound
    assert proben_amd._lib.lib().pe_version() >= 1


def test_product_path_refuses_cpu_tensors(built_lib):
    import torch
    import proben_amd
    import proben_amd.fusion as F
    z = torch.zeros((0, 4), dtype=torch.float64)
    with pytest.raises(proben_amd._lib.HipLibraryError):
        F.fuse_batch(z, z[:, 0], z[:, :3], z[:, 0], z[:, 0].int(), torch.zeros(1, dtype=torch.int32))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "multimodal-object-detection-via-probabilistic-ensembling_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f


def test_argument_checks_answer_before_any_device_work(built_lib):
    """Error behaviour of the C-ABI without a GPU: argument checks come first and explain themselves through pe_last_error()
    (null pointers, misaligned flat buffers of the fused SGD step, a ROI order workspace that is missing, bad stream counts)."""
    import proben_amd
    L = proben_amd._lib.lib()
    err = lambda: L.pe_last_error().decode()
    assert L.pe_sgd_momentum_f32(None, None, None, None, 0, 0.1, 0.9, 0.0, 1.0, 1, None) == 0          # empty range: nothing to do
    assert L.pe_sgd_momentum_f32(None, None, None, None, 8, 0.1, 0.9, 0.0, 1.0, 1, None) != 0 and "null pointer" in err()
    assert L.pe_sgd_momentum_f32(4096 + 8, 4096, 4096, None, 8, 0.1, 0.9, 0.0, 1.0, 1, None) != 0 and "16-byte aligned" in err()
    assert L.pe_sgd_momentum_f32(4096, 4096, 4096, 4096 + 4, 8, 0.1, 0.9, 0.0, 1.0, 1, None) != 0 and "16-byte aligned" in err()
    feats = (ctypes.c_void_p * 4)(4096, 4096, 4096, 4096)
    hw = (ctypes.c_int32 * 8)(200, 256, 100, 128, 50, 64, 25, 32)
    sc = (ctypes.c_float * 4)(0.25, 0.125, 0.0625, 0.03125)
    st = L.pe_roi_align_nhwc_sorted(feats, hw, sc, 4, 2, 256, 0, 4096, 1000, None, 7, 7, 0, 1, 4096, None, None, None)
    assert st != 0 and "order workspace" in err()


def declared_prototypes():
    """name -> the ctypes kind of every parameter, read from the prototypes of include/proben_hip.h (a pointer of any type is c_void_p)."""
    kinds = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "float": ctypes.c_float,
             "size_t": ctypes.c_size_t}
    txt = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(ROOT, "include", "proben_hip.h")).read(), flags=re.S)
    protos = {}
    for name, params in re.findall(r"\b(?:int|size_t|const\s+char\s*\*)\s*(pe_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        params = [p.split() for p in params.split(",") if p.strip() and p.strip() != "void"]
        protos[name] = [ctypes.c_void_p if any("*" in tok for tok in p) else kinds[p[-2]] for p in params]
    return protos


def test_python_signatures_have_the_headers_arity_and_kinds():
    """Every prototype of the header against _lib.SIGNATURES: the same number of parameters, and pointer -> c_void_p, int32_t -> c_int32,
    int64_t -> c_int64, double -> c_double, float -> c_float, size_t -> c_size_t in the same places.  The fusion's five signatures are
    derived from one table (_lib.FUSE_FIELDS); this holds them to the header like the hand-written ones."""
    import proben_amd
    protos = declared_prototypes()
    assert set(protos) == set(declared_symbols()) and len(protos) >= 58, set(declared_symbols()) ^ set(protos)
    sigs = dict(proben_amd._lib.SIGNATURES, pe_last_error=[])
    wrong = {n: (len(sigs[n]), len(p)) if len(sigs[n]) != len(p) else [i for i, (a, b) in enumerate(zip(sigs[n], p)) if a is not b]
             for n, p in protos.items() if list(sigs[n]) != p}
    assert not wrong, wrong
