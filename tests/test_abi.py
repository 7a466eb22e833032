"""The drop-in boundary: libnprealign.so loads, exports every symbol include/nprealign.h declares, and fails
loudly (no CPU fallback) when there is no GPU.  No compute calls here."""
import ctypes
import os
import re

import pytest

from helpers import ROOT
from nanopore_amd import _lib


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "nprealign.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(npr_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    L = _lib.load()
    declared = _declared_symbols()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(L, name), "libnprealign.so does not export %s" % name
    assert sorted(_lib.EXPORTS) == declared            # the binding covers the whole header
    assert L.npr_abi_version() == 1


def test_struct_layouts_match_the_header():
    assert ctypes.sizeof(_lib.Params) == 64
    assert ctypes.sizeof(_lib.ReadResult) == 56 and _lib.RESULT_DTYPE.itemsize == 56
    assert ctypes.sizeof(_lib.BatchStats) == 64


def test_error_strings():
    for code in range(0, -10, -1):
        assert _lib.strerror(code) and _lib.strerror(code) != "unknown error"
    assert _lib.strerror(-99) == "unknown error"


def test_no_cpu_fallback_without_a_gpu():
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        pytest.skip("a GPU is present: the failure path is exercised on the CPU box")
    from nanopore_amd import realign
    with pytest.raises(_lib.NprError) as e:
        realign.Context(0)
    assert e.value.code == _lib.ERR_NO_DEVICE
    assert "no CPU fallback" in str(e.value)


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under nanopore_amd/ or scripts/ may reference it."""
    bad = []
    for base in ("nanopore_amd", "scripts"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith((".py", ".cpp", ".h", ".hip")):
                    src = open(os.path.join(dirpath, f), errors="replace").read()
                    if re.search(r"^\s*(from|import)\s+oracle\b|liboracle|realign_oracle\.h", src, flags=re.M):
                        bad.append(os.path.join(dirpath, f))
    assert not bad, bad


def test_signature_table_covers_the_header_and_leaves_nothing_unspecified():
    """One table is the binding's whole knowledge of the ABI: a symbol without an entry would get ctypes' int return type (an int64_t
    truncated) and unchecked arguments."""
    assert set(_lib.SIGNATURES) == set(_declared_symbols()) and sorted(_lib.EXPORTS) == sorted(_lib.SIGNATURES)
    L = _lib.load()
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        assert restype is None or (isinstance(restype, type) and issubclass(restype, ctypes._SimpleCData)), name
        assert isinstance(argtypes, list), name   # [] for (void); never None, which ctypes reads as "anything goes"
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes, name


def test_check_raises_on_negative_codes_only():
    class Ctx(object):
        def last_error(self):
            return "what the context said"

    for rc in (0, 1, 19, 1 << 40):
        assert _lib.check(rc, "npr_somewhere") == rc and _lib.check(rc, "npr_somewhere", Ctx()) == rc
    with pytest.raises(_lib.NprError) as e:
        _lib.check(-1, "npr_somewhere")
    assert e.value.code == -1 and "npr_somewhere" in str(e.value) and "what the context said" not in str(e.value)
    with pytest.raises(_lib.NprError) as e:
        _lib.check(_lib.ERR_STATE, "npr_somewhere", Ctx())
    assert e.value.code == _lib.ERR_STATE and "npr_somewhere" in str(e.value) and "what the context said" in str(e.value)


def test_plan_handles_are_destroyed_exactly_once(monkeypatch):
    from nanopore_amd import realign as R
    L = _lib.load()
    destroy, destroyed = L.npr_plan_destroy, []
    monkeypatch.setattr(L, "npr_plan_destroy", lambda h: (destroyed.append(h.value), destroy(h)))
    P, guide = R.make_params(band_mode=R.BAND_FIXED, fixed_width=4), [(_lib.OP_M, 4)]
    segs = R.plan(P, 4, 4, guide)
    assert len(segs) == 1 and (segs[0]["xs"], segs[0]["ys"], segs[0]["xe"], segs[0]["ye"]) == (0, 0, 4, 4)
    assert len(destroyed) == 1 and destroyed[0]
    assert R.frame_schedule(P, 4, 4, guide, 64, 1)["cells"] > 0
    assert len(destroyed) == 2 and destroyed[1]
    assert len(R.stripes(P, 4, 4, guide)["X"]) == 1
    assert len(destroyed) == 3 and destroyed[2]
    with pytest.raises(_lib.NprError):   # (a segment the plan does not have: the handle goes all the same)
        R.stripes(P, 4, 4, guide, segment=1)
    assert len(destroyed) == 4 and destroyed[3]


def test_csr_helper_hands_over_the_same_bytes_padded_or_not():
    import numpy as np
    from nanopore_amd import realign as R
    mixed = ["ACGT", b"", b"NN", np.frombuffer(b"acg", dtype=np.uint8), ""]
    for items, text, off in (([], b"", [0]), ([b""], b"", [0, 0]), (mixed, b"ACGTNNacg", [0, 4, 4, 6, 9, 9])):
        for pad in (False, True):
            buf, o = R._csr(items, pad=pad)
            assert buf.dtype == np.uint8 and o.dtype == np.int64 and o.tolist() == off
            assert bytes(buf) == (text or (b"\0" if pad else b""))   # one zero byte where the join is empty: never a null pointer
        buf, o = R._ragged(items)
        assert bytes(buf) == (text or b"\0") and o.tolist() == off
